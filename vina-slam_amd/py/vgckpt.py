"""Checkpoint files (vg_checkpoint_save) read without the library: the header,
the section table and every section's checksum, recomputed with numpy. An
independent restatement of the file's rules (csrc/ckpt_file.h), so it pins the
device's checksum kernel (csrc/checkpoint.hip k_ckpt_sum).

    head | vg_config bytes | table[nsec] | pad to 16 | image

Checksum of a section: its bytes as little-endian 64-bit words, the last one
zero-padded; sum over i of word[i] * (MUL * (2 i + 1)) mod 2^64.
"""
import ctypes

import numpy as np

from vgconfig import CConfig

MAGIC = b"VINACKPT"
VERSION = 1
MUL = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1

HEAD = np.dtype([("magic", "S8"), ("version", "<u4"), ("nsec", "<u4"), ("cfg_bytes", "<u4"), ("head_bytes", "<u4"),
                 ("image_bytes", "<u8"), ("head_sum", "<u8"),
                 ("n_nodes", "<i4"), ("n_fix", "<i4"), ("n_slide", "<i4"), ("n_roots", "<i4"),
                 ("W", "<i4"), ("cap_wp", "<i4"), ("max_layer", "<i4"), ("pad", "<i4"),
                 ("wpn", "<i4", 32), ("arena", "<i4", 32), ("ord0", "<i4", 32)])
SEC = np.dtype([("id", "<u4"), ("rec", "<u4"), ("off", "<u8"), ("bytes", "<u8"), ("count", "<u8"), ("sum", "<u8")])
NAMES = ("?", "hdr", "plane", "pcr_add", "pcr_fix", "cov_add", "eig", "jour", "dbox", "pcrs", "lseg", "in_slide",
         "slide", "fix_pnt", "fix_var", "wp_pnt", "wp_var", "wp_leaf", "wp_int", "wp_ord", "slots", "root_id",
         "root_key", "dstate", "host")
NODE_SECTIONS = ("hdr", "plane", "pcr_add", "pcr_fix", "cov_add", "eig", "jour", "dbox", "pcrs", "lseg", "in_slide")
WINDOW_SECTIONS = ("wp_pnt", "wp_var", "wp_leaf", "wp_int")
HEAD_SUM_AT = 32  # offset of head_sum


class CkptError(ValueError):
    pass


def checksum(data):
    """The section checksum of a bytes-like object (any length)."""
    b = bytes(data)
    if len(b) % 8:
        b += b"\0" * (8 - len(b) % 8)
    w = np.frombuffer(b, dtype="<u8")
    if w.size == 0:
        return 0
    with np.errstate(over="ignore"):
        mul = (np.arange(w.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * np.uint64(MUL)
        return int((w * mul).sum(dtype=np.uint64))


def head_bytes(nsec):
    return (HEAD.itemsize + ctypes.sizeof(CConfig) + nsec * SEC.itemsize + 15) & ~15


def read(path_or_bytes):
    """(head record, config bytes, section table, image bytes); CkptError names the failed check."""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    raw = bytes(raw)
    if len(raw) < HEAD.itemsize:
        raise CkptError("file length (shorter than the header)")
    h = np.frombuffer(raw[: HEAD.itemsize], dtype=HEAD)[0]
    if h["magic"] != MAGIC:
        raise CkptError("magic")
    if h["version"] != VERSION:
        raise CkptError("version")
    csz = ctypes.sizeof(CConfig)
    if h["cfg_bytes"] != csz:
        raise CkptError("config size")
    nsec = int(h["nsec"])
    if nsec == 0 or nsec > 64 or int(h["head_bytes"]) != head_bytes(nsec):
        raise CkptError("section table (count / header size)")
    hb = int(h["head_bytes"])
    if len(raw) < hb:
        raise CkptError("file length (section table truncated)")
    if int(h["image_bytes"]) != len(raw) - hb:
        raise CkptError("file length")
    hz = bytearray(raw[:hb])
    hz[HEAD_SUM_AT: HEAD_SUM_AT + 8] = b"\0" * 8
    if checksum(hz) != int(h["head_sum"]):
        raise CkptError("header checksum")
    cfg = raw[HEAD.itemsize: HEAD.itemsize + csz]
    tab = np.frombuffer(raw[HEAD.itemsize + csz: HEAD.itemsize + csz + nsec * SEC.itemsize], dtype=SEC)
    end = 0
    for s in tab:
        off, nb = int(s["off"]), int(s["bytes"])
        if int(s["id"]) == 0 or int(s["id"]) >= len(NAMES):
            raise CkptError("section table (unknown id)")
        if nb != int(s["count"]) * int(s["rec"]):
            raise CkptError("section table (%s: byte count)" % NAMES[int(s["id"])])
        if off % 16 or off < end or off + nb > int(h["image_bytes"]):
            raise CkptError("section table (%s: out of the image's bounds)" % NAMES[int(s["id"])])
        end = off + nb
    return h, cfg, tab, raw[hb:]


def sections(path_or_bytes):
    """{name: (record bytes, count, payload bytes, stored checksum)}."""
    h, cfg, tab, img = read(path_or_bytes)
    return {NAMES[int(s["id"])]: (int(s["rec"]), int(s["count"]), img[int(s["off"]): int(s["off"]) + int(s["bytes"])],
                                  int(s["sum"])) for s in tab}


def verify(path_or_bytes):
    """Recompute every section's checksum; returns the head record and {name: (rec, count, checksum)}.
    CkptError on the first mismatch."""
    h, cfg, tab, img = read(path_or_bytes)
    out = {}
    for s in tab:
        name = NAMES[int(s["id"])]
        got = checksum(img[int(s["off"]): int(s["off"]) + int(s["bytes"])])
        if got != int(s["sum"]):
            raise CkptError("checksum of section %s: stored %016x, recomputed %016x" % (name, int(s["sum"]), got))
        out[name] = (int(s["rec"]), int(s["count"]), got)
    return h, out
