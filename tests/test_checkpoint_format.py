"""The checkpoint file's rules on the CPU (no GPU, no library call): vgckpt's
numpy checksum against a plain Python-integer loop, the position weighting
that makes a swapped pair of words visible, the reader's rejection of
truncated and over-long section tables, and the C++ validator
(csrc/ckpt_file.cpp) as a stand-alone program under AddressSanitizer and
UBSan, fed the malformed files of tests/test_checkpoint_gpu.py's test 5."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vgckpt
import vgpu
from vgconfig import CConfig

M64 = (1 << 64) - 1


def _loop_sum(b):
    """The rule restated with Python integers, byte by byte."""
    b = bytes(b) + b"\0" * (-len(b) % 8)
    acc = 0
    for i in range(len(b) // 8):
        w = int.from_bytes(b[8 * i: 8 * i + 8], "little")
        acc = (acc + w * ((vgckpt.MUL * (2 * i + 1)) & M64)) & M64
    return acc


@pytest.mark.parametrize("nbytes", [0, 1, 7, 8, 9, 13, 16, 24, 100, 1021, 4096 + 4])
def test_checksum_matches_integer_loop(nbytes):
    """Zero length, lengths that are no multiple of the 8-byte word or of the
    16-byte vector the device loads, and a few ordinary ones."""
    rng = np.random.default_rng(nbytes)
    b = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    assert vgckpt.checksum(b) == _loop_sum(b)
    assert (nbytes == 0) == (vgckpt.checksum(b) == 0) or nbytes > 0


def test_swapped_words_change_the_checksum():
    """Order-independent to compute, not order-blind: the sum of the words is
    the same after a swap, the position-weighted sum is not."""
    rng = np.random.default_rng(7)
    w = rng.integers(0, 1 << 63, 64, dtype=np.uint64)
    base = vgckpt.checksum(w.tobytes())
    for i, j in [(0, 1), (0, 63), (17, 18), (5, 40)]:
        v = w.copy()
        v[i], v[j] = w[j], w[i]
        assert int(v.sum(dtype=np.uint64)) == int(w.sum(dtype=np.uint64))
        assert vgckpt.checksum(v.tobytes()) != base, (i, j)
    # the same words in any order of summation give the same checksum (a plain reduction)
    perm = rng.permutation(64)
    mul = (np.arange(64, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * np.uint64(vgckpt.MUL)
    with np.errstate(over="ignore"):
        assert int((w * mul)[perm].sum(dtype=np.uint64)) == base


def _make_file(payloads):
    """A well-formed file of the given {section id: bytes} (counts are not checked by vgckpt.read)."""
    nsec = len(payloads)
    hb = vgckpt.head_bytes(nsec)
    tab = np.zeros(nsec, dtype=vgckpt.SEC)
    img = bytearray()
    for k, (sid, b) in enumerate(sorted(payloads.items())):
        tab[k] = (sid, 1, len(img), len(b), len(b), vgckpt.checksum(b))
        img += b + b"\0" * (-len(b) % 16)
    h = np.zeros(1, dtype=vgckpt.HEAD)
    h["magic"], h["version"], h["nsec"] = vgckpt.MAGIC, vgckpt.VERSION, nsec
    h["cfg_bytes"], h["head_bytes"], h["image_bytes"] = ctypes.sizeof(CConfig), hb, len(img)
    head = bytearray(hb)
    body = h.tobytes() + bytes(ctypes.sizeof(CConfig)) + tab.tobytes()
    head[: len(body)] = body
    h["head_sum"] = vgckpt.checksum(head)
    head[: vgckpt.HEAD.itemsize] = h.tobytes()
    return bytes(head) + bytes(img)


def _reseal(raw, nsec):
    """The header rewritten for another section count, with a matching header checksum."""
    h = np.frombuffer(raw[: vgckpt.HEAD.itemsize], dtype=vgckpt.HEAD).copy()
    h["nsec"], h["head_sum"] = nsec, 0
    hb = int(h["head_bytes"][0])
    head = bytearray(raw[:hb])
    head[: vgckpt.HEAD.itemsize] = h.tobytes()
    h["head_sum"] = vgckpt.checksum(head)
    head[: vgckpt.HEAD.itemsize] = h.tobytes()
    return bytes(head) + raw[hb:]


def test_reader_accepts_and_rejects():
    good = _make_file({1: b"abc" * 11, 2: b"", 7: bytes(range(64))})
    h, secs = vgckpt.verify(good)
    assert secs["hdr"][1] == 33 and secs["plane"][1] == 0 and secs["jour"][2] == vgckpt.checksum(bytes(range(64)))
    # truncated and over-long section tables, with and without a matching header checksum
    for nsec in (0, 2, 4, 65, 1 << 31):
        bad = bytearray(good)
        bad[12:16] = int(nsec).to_bytes(4, "little")
        with pytest.raises(vgckpt.CkptError, match="section table"):
            vgckpt.read(bytes(bad))
        with pytest.raises(vgckpt.CkptError, match="section table"):
            vgckpt.read(_reseal(good, nsec))
    for cut in (1, 16, len(good) - 100, len(good)):
        with pytest.raises(vgckpt.CkptError, match="file length"):
            vgckpt.read(good[: len(good) - cut])
    with pytest.raises(vgckpt.CkptError, match="file length"):
        vgckpt.read(good + b"\0")
    with pytest.raises(vgckpt.CkptError, match="magic"):
        vgckpt.read(b"X" + good[1:])
    flip = bytearray(good)
    flip[-40] ^= 1
    with pytest.raises(vgckpt.CkptError, match="checksum of section jour"):
        vgckpt.verify(bytes(flip))
    # a table entry pointing out of the image
    hb = int(h["head_bytes"])
    at = vgckpt.HEAD.itemsize + ctypes.sizeof(CConfig) + vgckpt.SEC.itemsize * 2 + 8  # third entry's offset
    bad = bytearray(good)
    bad[at: at + 8] = (len(good) - hb + 16).to_bytes(8, "little")
    with pytest.raises(vgckpt.CkptError, match="header checksum"):
        vgckpt.read(bytes(bad))
    with pytest.raises(vgckpt.CkptError, match="out of the image"):
        vgckpt.read(_reseal(bytes(bad), 3))


def test_validator_under_sanitizers(tmp_path):
    """The C++ reader / validator, stand-alone, under ASan + UBSan: its
    self-test feeds it a flipped payload byte, truncations, a bad magic,
    another configuration, truncated and over-long section tables and table
    entries out of bounds; every case must be rejected with the right check
    and no sanitizer report (a report aborts: non-zero exit)."""
    exe = str(tmp_path / "ckpt_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(vgpu.PKG, "tools", "ckpt_check.cpp"),
                           os.path.join(vgpu.PKG, "csrc", "ckpt_file.cpp")])
    out = subprocess.run([exe, "--selftest"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "selftest ok" in out.stdout and "FAILED" not in out.stdout
    # the two readers agree on a file neither wrote for the other: the C++ tool rejects vgckpt's
    # synthetic file at the section table (its sections are not a context's), not at the header checksum
    p = tmp_path / "synthetic.vgck"
    p.write_bytes(_make_file({1: b"abc" * 32}))
    out = subprocess.run([exe, str(p)], capture_output=True, text=True)
    assert out.returncode == 1 and "dimensions" in out.stdout, out.stdout + out.stderr
