"""The insert chain that counts its buckets in the descent (vgx_debug 38:
prep -> roots -> descend + counts -> alloc || segment allocation -> scatter ->
push, six launches) and k_push_window's pipelined record loads and LDS ranking
(vgx_debug 39), against their earlier forms (k_ins_resolve + k_seg_offsets +
k_ins_scatter; loads in series with the sums), bit for bit; the host-sized
insert replay behind the new chain; and the shapes the new code branches on
(skip path, leaf sizes around 64 and kPwRankMax, several children under one
parent), checked against the oracle."""
import ctypes

import numpy as np
import pytest

import oracle
import synth
import vgconfig
import vgpu

import insert_edge_input as E

pytestmark = pytest.mark.gpu
CAP = dict(max_points=120_000, max_nodes=600_000, max_fix_points=2_000_000, hash_log2=20)
COUNTERS = ("n_raw", "n_ds", "iekf_iters", "iekf_matches", "roots_new", "n_slide", "n_factors", "ba_iters",
            "degenerate", "plane_updates", "fix_full")
K_PW_RANK_MAX = 256  # insert.hip kPwRankMax


def _seq(p, lidar="16line", seq_id=4):
    g = p["General"]
    return synth.Sequence(lidar, seq_id, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])


def _pair(ka, kb, seq_id, nscan):
    p = vgconfig.load("mid360")
    seq = _seq(p, seq_id=seq_id)
    a = vgpu.Context(vgconfig.to_c(p), **CAP)
    b = vgpu.Context(vgconfig.to_c(p), **CAP)
    for c, kv in ((a, ka), (b, kb)):
        # two live contexts on the device turn the flag hand-offs off unless forced:
        # each context is drained (stats) before the other steps
        for key, val in {14: 2, **kv}.items():
            assert vgpu.lib().vgx_debug(c.h, key, val) == 0
    a.seed(seq.gt_state(0))
    b.seed(seq.gt_state(0))
    for k in range(nscan):
        xyz, it, beg, end = seq.scan(k)
        imu = seq.imu(k)
        a.step(xyz, it, beg, end, imu)
        b.step(xyz, it, beg, end, imu)
        sa, sb = a.stats(), b.stats()
        assert sa == sb, (k, sa, sb)
    assert np.array_equal(a.trajectory(), b.trajectory())
    assert np.array_equal(a.window_states(), b.window_states())
    a.close()
    b.close()


@pytest.mark.parametrize("ka,kb", [({38: 0}, {38: 1}), ({39: 0}, {39: 1}), ({38: 0, 39: 0}, {38: 1, 39: 1}),
                                   ({38: 0, 39: 1}, {38: 1, 39: 0})],
                         ids=["counts-in-descent", "push-window-pipelined", "both", "crossed"])
def test_insert_switch_on_equals_off(ka, kb):
    """Each new switch off against on: stats equal per scan, trajectory and
    window states bit for bit, 15 scans (the sequence and capacities of
    test_fused_launches_equal_separate)."""
    _pair(ka, kb, seq_id=7, nscan=15)


def test_insert_replay_behind_counted_descent():
    """vgx_debug(3, 0): every child allocation overflows k_ins_alloc, the host
    creates the children and the new tail (scatter + push) runs on the
    segments and request counts the aborted insert left; bit for bit the fast
    path, 14 scans."""
    _pair({38: 1}, {38: 1, 3: 0}, seq_id=6, nscan=14)


# ---------------------------------------------------------------- edge shapes
def _segments(ctx):
    """The last insert's segments (test hook): keys (a leaf id, or a child
    request -2 - (parent * 8 + octant)), lengths, and [segments, roots touched,
    parents with requests, abort flag]."""
    L = vgpu.lib()
    L.vgx_insert_segments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p]
    L.vgx_insert_segments.restype = ctypes.c_int
    cap = 200_000
    key = np.zeros(cap, np.int32)
    ln = np.zeros(cap, np.int32)
    info = np.zeros(4, np.int32)
    assert L.vgx_insert_segments(ctx.h, key.ctypes.data, ln.ctypes.data, cap, info.ctypes.data) == 0
    n = int(info[0])
    assert n <= cap
    return key[:n].copy(), ln[:n].copy(), info


@pytest.mark.parametrize("pipe", [0, 1], ids=["loads-in-series", "loads-pipelined"])
def test_insert_edge_shapes_match_oracle(oracle_lib, pipe):
    """The shapes the counted descent and k_push_window branch on, in one short
    sequence (insert_edge_input.py): a scan on the skip path and a normal one
    after it; leaves receiving exactly 1, 64, 65, kPwRankMax, kPwRankMax + 1
    and 320 points in one scan; children created under one existing parent in
    several octants at once. Each precondition is asserted from the device's
    own segments (vgx_insert_segments, read right after the insert); every
    counter equals the oracle's and the poses agree within 1e-9 m."""
    p = E.config(vgconfig)
    seq, scans, keys = E.make(p)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0))
    gpu = vgpu.Context(vgconfig.to_c(p), **CAP)
    for key, val in ((38, 1), (39, pipe)):
        assert vgpu.lib().vgx_debug(gpu.h, key, val) == 0
    orc.seed(seq.gt_state(0))
    gpu.seed(seq.gt_state(0))
    W = p["LocalBA"]["win_size"]
    thread_num = p["LocalBA"]["thread_num"]
    seen_lengths, octants_at_once = set(), 0
    for k, (xyz, it, beg, end, imu) in enumerate(scans):
        orc.step(xyz, it, beg, end, imu)
        gpu.scan_load(xyz, it)
        gpu.propagate(imu, beg, end)
        gpu.downsample_scan()
        gpu.lio_state_estimation()
        gpu.window_push(imu)
        gpu.cut_voxel_multi()
        key, ln, info = _segments(gpu)
        gpu.multi_recut()
        if gpu.win_count() >= W:
            gpu.damping_iter()
            gpu.multi_margi()
        gpu.step_end()
        so, sg = orc.stats(), gpu.stats()
        for c in COUNTERS:
            assert so[c] == sg[c], (k, c, so[c], sg[c])
        print(k, "segments", info[0], "roots touched", info[1], "parents with requests", info[2])
        if k == 0:  # the skip path: fewer than thread_num roots, no segment at all
            assert 0 < info[1] < thread_num and info[0] == 0 and sg["n_ds"] > 0
        else:
            assert info[1] >= thread_num and info[0] > 0 and info[3] == 0
            assert int(ln.sum()) == sg["n_ds"] and ln.min() >= 1
        if k == 1:
            seen_lengths = set(int(x) for x in ln)
        req = -2 - key[key < -1]
        if req.size:
            parents, n_oct = np.unique(req >> 3, return_counts=True)
            octants_at_once = max(octants_at_once, int(n_oct.max()))
    for want in E.SIZES:
        assert want in seen_lengths, (want, sorted(seen_lengths)[-12:])
    assert max(E.SIZES) >= 300 and K_PW_RANK_MAX in E.SIZES and K_PW_RANK_MAX + 1 in E.SIZES
    assert octants_at_once >= 2, octants_at_once
    to, tg = orc.trajectory(), gpu.trajectory()
    dpos = np.linalg.norm(to[:, 10:13] - tg[:, 10:13], axis=1).max()
    print("max dpos %.3e m" % dpos)
    assert dpos < 1e-9 and np.abs(to[:, 1:10] - tg[:, 1:10]).max() < 1e-9
    assert np.abs(orc.window_states()[:, 1:25] - gpu.window_states()[:, 1:25]).max() < 1e-9
    gpu.close()
    orc.close()
