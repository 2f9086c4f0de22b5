"""bench.py's plain run and --dump-outputs (one small run: config 2, 3 steps).

A plain run prints the headline line without the figures that need runs of
their own (those are --full's), really times --steps steps, and
--dump-outputs writes what the last timed pass computed: the arrays a caller
of BundleAdjuster.step holds afterwards.  They are compared with the same pass
made here, on the same seeded scene -- the inputs bit for bit, the results
to the bounds tests/test_gpu_dist.py uses between two summation orders (SSE
1e-12, da / db 1e-6 of their largest entry).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("phases_ms", "roofline", "solve_roofline", "cpu_baseline", "other_configs")


@pytest.mark.timeout(240)
def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    from bundleadjustmentmatlab_amd.scene import make_config
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--config", "cfg2", "--steps", "3", "--warmup", "1",
                        "--clock-ramp", "0.02", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [q for q in r.stdout.splitlines() if q.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "LM iterations/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["metric"]
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    assert not [k for k in FULL_ONLY if k in line], line.keys()

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["a", "b", "da", "db", "step_info"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20

    sc = make_config("cfg2", gpu=True, device=0)
    a0 = np.vstack([sc.w0, sc.T0])
    b0 = np.asfortranarray(sc.X0[:3])
    with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6) as ba:
        ba.set_params(a0, b0)
        info = ba.step(relinearize=True, update_lm=False)
        da, db = ba.last_step()
    assert np.array_equal(got["a"], a0) and np.array_equal(got["b"], b0)
    old, new = got["step_info"][:2]
    print(f"old_sse {old!r} vs {info.old_sse!r}, new_sse {new!r} vs {info.new_sse!r}, "
          f"da bitwise {np.array_equal(got['da'], da)}, db bitwise {np.array_equal(got['db'], db)}")
    assert got["step_info"].shape == (10,)
    assert abs(old - info.old_sse) <= 1e-12 * info.old_sse
    assert abs(new - info.new_sse) <= 1e-12 * info.new_sse
    assert got["da"].shape == (6, sc.m) and got["db"].shape == (3, sc.n)
    assert np.abs(got["da"] - da).max() <= 1e-6 * np.abs(da).max()
    assert np.abs(got["db"] - db).max() <= 1e-6 * np.abs(db).max()
