"""The host planners' test problems and their stand-alone harnesses, shared by
test_plan_threads.py, test_plan_sanitize.py and test_solve_plan.py:
tools/bench_plan.cpp + csrc/ba_plan.cpp, and tools/bench_chol_plan.cpp with
csrc/ba_chol_plan.cpp beside them, built with the host C++ compiler (no ROCm),
and the problem files they read."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "g++"
SOURCES = [os.path.join(ROOT, "tools", "bench_plan.cpp"),
           os.path.join(ROOT, "bundleadjustmentmatlab_amd", "csrc", "ba_plan.cpp")]
CHOL_SOURCES = [os.path.join(ROOT, "tools", "bench_chol_plan.cpp"), SOURCES[1],
                os.path.join(ROOT, "bundleadjustmentmatlab_amd", "csrc", "ba_chol_plan.cpp")]
CASES = ["cfg5x_300", "ladybug_small", "banded", "ladder6_257", "ladder12_280", "shared_257"]
# ... and the smallest problems that reach the solve paths those six miss
# (test_solve_plan.py): camera-aligned cyclic reduction at num_a 7 / 10 / 12,
# 64-row cyclic reduction, two camera groups that share no point, one tile
BANDED = {"cr_track5": dict(m=90, n=3600, track=5, seed=41),
          "cr_track4": dict(m=90, n=3600, track=4, seed=41),
          "cr_track3": dict(m=90, n=3600, track=3, seed=41),
          "cr64_track9": dict(m=64, n=2560, track=9, seed=41),
          "tiny10": dict(m=10, n=400, track=4, seed=41)}
SOLVE_CASES = CASES + sorted(BANDED) + ["two_groups"]


def golden():
    """{name: {"hash", "m", "n", "N"}} recorded from the planner (plan_hashes.json)."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_hashes.json")) as f:
        return json.load(f)


def build_harness(exe, flags=("-O2",), sources=SOURCES):
    return subprocess.run([CXX, "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"),
                           "-pthread", *sources, "-o", str(exe)], capture_output=True, text=True)


def write_case(name, path):
    """Write problem `name` (int32 m, n, N, obs_pt[N], obs_cam[N]); returns (m, n, N)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bundleadjustmentmatlab_amd.scene import make_config
    if name in ("ladder6_257", "ladder12_280", "shared_257"):
        # tests/track_scenes.py: tracks on every length threshold up to three
        # full segments; 257 long tracks through the same 90 cameras
        import track_scenes as ts
        sc, pt, cam, _ = {"ladder6_257": lambda: ts.ladder(6, 257),
                          "ladder12_280": lambda: ts.ladder(12, 280),
                          "shared_257": lambda: ts.shared(257)}[name]()
        m, n = sc.m, sc.n
    elif name == "cfg5x_300":    # short, per-term and long tracks (up to 76 views), re-detections
        from prof_cfg5x_solve import sub_problem
        sc = make_config("cfg5x")
        used, pt, cam, _ = sub_problem(sc, 300)
        m, n = 300, len(used)
    elif name == "ladybug_small":   # loop closures + long tracks past a chunk (segment chunks)
        sc = make_config("ladybug", m=200, n=20_000, long_frac=0.01, long_len=(130, 180))
        m, n, pt, cam = sc.m, sc.n, sc.obs_pt, sc.obs_cam
    elif name in BANDED:
        sc = make_config("cfg2", **BANDED[name])
        m, n, pt, cam = sc.m, sc.n, sc.obs_pt, sc.obs_cam
    elif name == "two_groups":   # cameras 0..59 and 60..119 never share a point
        rng = np.random.default_rng(7)
        m, n = 120, 1200
        pt = np.repeat(np.arange(n), 4)
        cam = np.concatenate([np.sort(rng.choice(60, 4, replace=False)) + 60 * (i % 2)
                              for i in range(n)])
    else:
        assert name == "banded"
        sc = make_config("cfg2")
        m, n, pt, cam = sc.m, sc.n, sc.obs_pt, sc.obs_cam
    with open(path, "wb") as f:
        np.array([m, n, len(pt)], np.int32).tofile(f)
        np.asarray(pt, np.int32).tofile(f)
        np.asarray(cam, np.int32).tofile(f)
    return m, n, len(pt)


def hashes(stdout):
    """The plan hash of every problem of one harness run, in order."""
    return re.findall(r"hash ([0-9a-f]{16})", stdout)
