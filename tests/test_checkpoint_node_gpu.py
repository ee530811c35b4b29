"""Checkpoint and resume at the node level: bin/vg_node_replay over the 16-line
event log of tests/test_node_core.py, once straight through, once with
--checkpoint-out / --checkpoint-at and then --resume in a second process. The
TUM file and the path output of the resumed run are byte-identical to the
uninterrupted run's: the TUM rows continue the saved ones."""
import json
import os
import subprocess

import pytest

import synth
import vgconfig
from test_node_core import REPO, _events, _fmt, _write_log

pytestmark = pytest.mark.gpu


def _replay(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_replay_resume_is_byte_identical(tmp_path):
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 12, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    log = tmp_path / "ev.bin"
    _write_log(log, vgconfig.to_c(p), _fmt(g["blind"]), seq.gt_state(0), _events(seq, 16))
    exe = os.path.join(REPO, "vina-slam_amd", "bin", "vg_node_replay")
    ck = tmp_path / "node.vgck"
    a = _replay(exe, [log, tmp_path / "a.tum", 0, tmp_path / "a.path"])
    assert a["stepped"] >= 14
    b = _replay(exe, [log, tmp_path / "b.tum", 0, tmp_path / "b.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    assert b["stepped"] == a["stepped"] and ck.exists() and int((tmp_path / "node.vgck.meta").read_text()) == 12
    c = _replay(exe, [log, tmp_path / "c.tum", 0, tmp_path / "c.path", "--resume", ck])
    assert c["stepped"] == a["stepped"] - 12 and c["poses"] == a["poses"] and c["path"] == a["path"]
    ref_tum, ref_path = (tmp_path / "a.tum").read_bytes(), (tmp_path / "a.path").read_bytes()
    assert len(ref_tum.splitlines()) == a["poses"] > 12
    for name in ("b", "c"):  # the saver is undisturbed, the resumed run continues the saved rows
        assert (tmp_path / (name + ".tum")).read_bytes() == ref_tum, name
        assert (tmp_path / (name + ".path")).read_bytes() == ref_path, name
