"""csrc/vg_scratch.h (DevBuf, KernelTimer) on the host, stand-alone under
ASan + UBSan: tools/scratch_check.cpp stubs the HIP entry points the header
calls over malloc / free, so no GPU, no HIP runtime and no Python take part in
the run."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "vina-slam_amd", "py"))

import vgpu  # noqa: E402


def test_scratch_types_under_sanitizers(tmp_path):
    """reserve within and past capacity, reserve_pow2's sequence, a failed
    reserve leaving the buffer empty and usable, moves freeing exactly once,
    the four-buffer staging whose third allocation fails and is retried (the
    leak of the hand-written info_bufs / ray_bufs), KernelTimer before begin
    and after its destruction. A sanitizer report, LeakSanitizer's at exit
    included, aborts: non-zero exit."""
    exe = str(tmp_path / "scratch_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-o", exe, os.path.join(vgpu.PKG, "tools", "scratch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scratch ok" in out.stdout and "FAILED" not in out.stdout
