"""The host planner's test problems and its stand-alone harness, shared by
test_plan_threads.py and test_plan_sanitize.py: tools/bench_plan.cpp +
csrc/ba_plan.cpp built with the host C++ compiler (no ROCm), and the problem
files it reads."""
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
CASES = ["cfg5x_300", "ladybug_small", "banded", "ladder6_257", "ladder12_280", "shared_257"]


def golden():
    """{name: {"hash", "m", "n", "N"}} recorded from the planner (plan_hashes.json)."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_hashes.json")) as f:
        return json.load(f)


def build_harness(exe, flags=("-O2",)):
    return subprocess.run([CXX, "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"),
                           "-pthread", *SOURCES, "-o", str(exe)], capture_output=True, text=True)


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
