#!/bin/bash
# Build tools/build/bench_plan (the CPU harness of the context's host planner:
# tools/bench_plan.cpp + csrc/ba_plan.cpp, host compiler only, with the
# planner's phase times on stderr) and tools/build/bench_chol_plan (the reduced
# solve's planner: tools/bench_chol_plan.cpp + csrc/ba_plan.cpp +
# csrc/ba_chol_plan.cpp), and write the problem files they read
# (tools/build/plan_*.bin).
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/build
${CXX:-c++} -O3 -std=c++17 -ffp-contract=off -DBA_PLAN_TIMING -I include -pthread \
  tools/bench_plan.cpp bundleadjustmentmatlab_amd/csrc/ba_plan.cpp -o tools/build/bench_plan
${CXX:-c++} -O3 -std=c++17 -ffp-contract=off -I include -pthread \
  tools/bench_chol_plan.cpp bundleadjustmentmatlab_amd/csrc/ba_plan.cpp \
  bundleadjustmentmatlab_amd/csrc/ba_chol_plan.cpp -o tools/build/bench_chol_plan
python3 - <<'PY'
import sys
import numpy as np
sys.path[:0] = [".", "tools"]
from bundleadjustmentmatlab_amd.scene import make_config
from prof_cfg5x_solve import sub_problem


def write(name, m, n, pt, cam):
    with open(f"tools/build/plan_{name}.bin", "wb") as f:
        np.array([m, n, len(pt)], np.int32).tofile(f)
        np.asarray(pt, np.int32).tofile(f)
        np.asarray(cam, np.int32).tofile(f)


sc = make_config("cfg5x")
for M in (300, 900):
    used, pt, cam, _ = sub_problem(sc, M)
    write(f"cfg5x_{M}", M, len(used), pt, cam)
for name in ("cfg2", "ladybug"):
    s = make_config(name)
    write(name, s.m, s.n, s.obs_pt, s.obs_cam)
s = make_config("cfg3")
write("cfg3", s.m, s.n, s.obs_pt, s.obs_cam)
PY
