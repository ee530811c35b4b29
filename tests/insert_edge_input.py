"""Input of the insert chain's edge-shape test (test_insert_chain_gpu.py): a
16-line sequence on mid360 parameters with 2 m root voxels, whose

* scan 0 is cut down to three points: fewer than thread_num roots, so the
  insert takes its skip path (voxel_map.cpp:96-97);
* scan 1 carries six blocks of points, each in the lower half of an otherwise
  empty root voxel, on a 0.18 m grid (two points 0.18 m apart never share a
  0.1 m downsample cell, whatever the frame), so the voxels' leaves receive
  exactly 1, 64, 65, kPwRankMax, kPwRankMax + 1 and 320 downsampled points;
* scan 3 adds a 10 x 10 layer across the four upper octants of the two largest
  blocks' voxels: once those leaves have subdivided, four children are created
  under one existing parent at once.
"""
import numpy as np

import synth

VOXEL = 2.0
GRID = 0.18
SIZES = (1, 64, 65, 256, 257, 320)
NSCAN = 6


def config(vgconfig):
    p = vgconfig.load("mid360")
    p["Odometry"]["voxel_size"] = VOXEL
    return p


def _to_lidar(seq, k, w):
    R, t = seq.gt_pose(k)
    return (((w - t[None, :]) @ R) - seq.ext_t[None, :]) @ seq.ext_R


def _world(seq, k, x):
    R, t = seq.gt_pose(k)
    return (x.astype(np.float64) @ seq.ext_R.T + seq.ext_t[None, :]) @ R.T + t[None, :]


def _block(lo, count, z0=0.19):
    k = np.arange(count)
    ijk = np.stack([k % 10, (k // 10) % 10, k // 100], 1).astype(np.float64)
    return lo[None, :] + np.array([0.19, 0.19, z0])[None, :] + GRID * ijk


def make(p):
    """[(xyz, intensity, beg, end, imu)] per scan, and the six root voxels
    (integer keys at VOXEL) holding the blocks, in SIZES order."""
    g = p["General"]
    seq = synth.Sequence("16line", 4, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    scans = [list(seq.scan(k)) + [seq.imu(k)] for k in range(NSCAN)]
    scans[0][0], scans[0][1] = np.ascontiguousarray(scans[0][0][:3]), np.ascontiguousarray(scans[0][1][:3])
    # root voxels no scan of the sequence touches, 4 - 15 m from every sensor position, inside the scene's box,
    # no two of them neighbours
    used = set()
    for k in range(NSCAN):
        used |= set(map(tuple, np.floor(_world(seq, k, seq.scan(k)[0]) / VOXEL).astype(int)))
    pos = np.array([seq.gt_pose(k)[1] for k in range(NSCAN)])
    keys = []
    for ix in range(-9, 9):
        for iy in range(-4, 4):
            for iz in (0, 1, 2):
                key = (ix, iy, iz)
                c = (np.array(key) + 0.5) * VOXEL
                d = np.linalg.norm(pos - c[None, :], axis=1)
                if d.min() > 4.0 and d.max() < 15.0 and key not in used and all(
                        max(abs(a - b) for a, b in zip(key, q)) > 1 for q in keys):
                    keys.append(key)
    keys = keys[:len(SIZES)]
    assert len(keys) == len(SIZES), keys
    for key, count in zip(keys, SIZES):
        w = _block(np.array(key, dtype=np.float64) * VOXEL, count)
        x = _to_lidar(seq, 1, w).astype(np.float32)
        scans[1][0] = np.ascontiguousarray(np.concatenate([scans[1][0], x]))
        scans[1][1] = np.ascontiguousarray(np.concatenate([scans[1][1], np.full(count, 7, np.float32)]))
    for key in keys[-2:]:
        w = _block(np.array(key, dtype=np.float64) * VOXEL, 100, z0=1.3)
        x = _to_lidar(seq, 3, w).astype(np.float32)
        scans[3][0] = np.ascontiguousarray(np.concatenate([scans[3][0], x]))
        scans[3][1] = np.ascontiguousarray(np.concatenate([scans[3][1], np.full(100, 7, np.float32)]))
    return seq, scans, keys
