"""csrc/vg_lm_loop.h (the LM's host loop, shared by ba_run and ba_resolve) on
the host, stand-alone under ASan + UBSan: tools/lm_loop_check.cpp drives it
against a scripted device, so no GPU, no HIP runtime and no Python take part in
the run."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "vina-slam_amd", "py"))

import vgpu  # noqa: E402


def test_lm_loop_under_sanitizers(tmp_path):
    """Every convergence iteration 1..10 and "never", every ba_last_iters
    1..10, pre in {0, 2}, the one-graph and two-graph starts, flags on time,
    early and late: (a) the launches and iters / tail_ok / ba_last_iters equal
    a literal restatement of ba_run's former loop, (b) a run deferred at its
    first opportunity and resolved, blocking or polling, gives the same, (c)
    early and late flags change no launch. A sanitizer report aborts: non-zero
    exit."""
    exe = str(tmp_path / "lm_loop_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(vgpu.PKG, "tools", "lm_loop_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lm loop ok" in out.stdout and "FAILED" not in out.stdout
