"""bench.py's command line: a plain run is the metric leg alone, --full switches
the other legs back on (and their selectors then hold), --dump-outputs writes
float64 .npy arrays."""
import numpy as np

import bench


def _legs(a):
    return (a.no_cpu, a.no_h2d, a.no_tile1, a.stage_scans, a.target_steps, a.multi, a.multi_1m)


def test_plain_run_is_the_metric_leg_alone():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, "")
    assert _legs(a) == (True, True, True, 0, 0, "", "")
    # the legs' own selectors mean nothing without --full
    a = bench.parse(["--stage-scans", "8", "--multi", "2,4", "--target-steps", "20"])
    assert _legs(a) == (True, True, True, 0, 0, "", "")


def test_full_runs_every_leg_and_keeps_the_selectors():
    a = bench.parse(["--full"])
    assert a.full and _legs(a) == (False, False, False, 8, 20, "2,4,8,16", "1,2,4,8")
    a = bench.parse(["--full", "--no-cpu", "--stage-scans", "0", "--multi=", "--multi-1m", "2"])
    assert _legs(a) == (True, False, False, 0, 20, "", "2")


def test_dump_outputs_writes_float64_arrays(tmp_path):
    class Ctx:
        def trajectory(self):
            return np.arange(26.0).reshape(2, 13)

        def path(self):
            return np.arange(28.0).reshape(2, 14)

        def state(self):
            return np.arange(250.0)

    stats = [{"n_raw": 5, "iekf_matches": [1, 2, 3, 4], "n_ds": 3}, {"n_raw": 6, "iekf_matches": [4, 3, 2, 1], "n_ds": 2}]
    out = tmp_path / "deep" / "dir"  # created on demand
    bench.dump_outputs(str(out), Ctx(), stats)
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["counters.npy", "path.npy", "state.npy", "trajectory.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["trajectory.npy"], Ctx().trajectory())
    assert np.array_equal(got["path.npy"], Ctx().path())
    assert np.array_equal(got["state.npy"], Ctx().state())
    assert np.array_equal(got["counters.npy"], [[5, 1, 2, 3, 4, 3], [6, 4, 3, 2, 1, 2]])
