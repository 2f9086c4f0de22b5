"""Host against GPU triangulation in the growing replay (cfg5x).

1. One replay whose replay-thread triangulations are timed both ways on the
   same arguments: incremental._triangulate (numpy, one padded batched SVD)
   against incremental._triangulate_gpu (bundle.triangulate_points: copies,
   two launches, copy back).  Reports per call the batch size, the longest
   track, host ms and GPU ms, and whether the two accept the same points.
2. Three ``triangulation="gpu"`` replays against three ``"host"`` ones,
   interleaved, on one box: wall seconds, the solves' and resections' seconds
   and the rest (the replay's host glue, as bench.py's host_device_split_s
   counts it).

usage: python tools/triangulate_time.py [M] [--out DIR] [--runs R]
Writes DIR/batches_m<M>.csv and DIR/replay_m<M>.json (default
profiles/triangulate)."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bundleadjustmentmatlab_amd.incremental as inc  # noqa: E402
from bundleadjustmentmatlab_amd.scene import make_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("m", nargs="?", type=int, default=1000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate"))
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
sc = make_config("cfg5x", m=args.m) if args.m != 1000 else make_config("cfg5x")
print(f"cfg5x m={sc.m} n={sc.n} obs={sc.num_obs}", flush=True)

# ---- 1. the replay thread's batches, both ways ---------------------------------
rows = []
host_tri = inc._triangulate


def both(sc_, K, T, w, pts, status):
    if threading.current_thread() is not threading.main_thread() or len(pts) == 0:
        return host_tri(sc_, K, T, w, pts, status)
    t0 = time.perf_counter()
    Xh = host_tri(sc_, K, T, w, pts, status)
    t1 = time.perf_counter()
    Xg = inc._triangulate_gpu(sc_, K, T, w, pts, status)
    t2 = time.perf_counter()
    sel = inc._tri_rows(sc_, pts, status)
    longest = int(np.bincount(np.searchsorted(pts, sc_.obs_pt[sel])).max())
    ok = Xh[3] == 1
    same = bool(np.array_equal(ok, Xg[3] == 1))
    dev = float(np.abs(Xg[:3, ok] - Xh[:3, ok]).max() /
                max(np.abs(Xh[:3, ok]).max(), 1e-300)) if same and ok.any() else float("nan")
    rows.append((len(pts), len(sel), longest, 1e3 * (t1 - t0), 1e3 * (t2 - t1), int(same), dev))
    return Xh


inc._triangulate = both
try:
    inc.incremental_bundle(sc, devices=[0])
finally:
    inc._triangulate = host_tri
r = np.array(rows)
with open(os.path.join(args.out, f"batches_m{sc.m}.csv"), "w") as f:
    f.write("points,views,longest_track,host_ms,gpu_ms,same_accepted_set,max_rel_diff\n")
    for q in rows:
        f.write("%d,%d,%d,%.4f,%.4f,%d,%.3e\n" % q)
batches = {
    "calls": len(rows),
    "points_median_max": [float(np.median(r[:, 0])), float(r[:, 0].max())],
    "longest_track_median_max": [float(np.median(r[:, 2])), float(r[:, 2].max())],
    "host_ms_total_median_max": [float(r[:, 3].sum()), float(np.median(r[:, 3])),
                                 float(r[:, 3].max())],
    "gpu_ms_total_median_max": [float(r[:, 4].sum()), float(np.median(r[:, 4])),
                                float(r[:, 4].max())],
    "same_accepted_set": int(r[:, 5].sum()),
    "max_rel_diff": float(np.nanmax(r[:, 6])),
}
print(json.dumps(batches), flush=True)

# ---- 2. whole replays, interleaved ---------------------------------------------
runs = []
for k in range(args.runs):
    for mode in ("host", "gpu"):
        t0 = time.perf_counter()
        res = inc.incremental_bundle(sc, devices=[0], triangulation=mode)
        wall = time.perf_counter() - t0
        sol = res["solves"]
        solves = sum(q["seconds"] for q in sol)
        resect = sum(q["seconds"] for q in res["resections"])
        runs.append({"mode": mode, "run": k, "wall_s": wall, "solves_s": solves,
                     "resections_s": resect, "host_glue_s": wall - solves - resect,
                     "wait_for_context_s": sum(q["wait_create"] for q in sol),
                     "final_error": float(sol[-1]["error"][-1]),
                     "reconstructed": int((res["X"][3] == 1).sum()),
                     "mispredicted": res["prefetch"]["mispredicted"]})
        print(json.dumps(runs[-1]), flush=True)
summary = {mode: {key: sorted(q[key] for q in runs if q["mode"] == mode)
                  for key in ("wall_s", "host_glue_s")} for mode in ("host", "gpu")}
with open(os.path.join(args.out, f"replay_m{sc.m}.json"), "w") as f:
    json.dump({"scene": {"config": "cfg5x", "m": sc.m, "n": sc.n, "observations": sc.num_obs},
               "batches": batches, "replays": runs, "sorted": summary}, f, indent=1)
print(json.dumps(summary))
