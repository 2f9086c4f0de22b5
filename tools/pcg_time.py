"""The block-Jacobi PCG reduced solve (solver="pcg") beside solver="auto" on
non-banded scenes, in one process, the variants alternating: untimed wall time
per relinearising pass (no kernel events, as tools/pass_time.py), the PCG's
iterations per pass, a whole run() of each to a final cost within 1e-6 of each
other, and the device memory the reduced solve holds (plan_info()["solve_bytes"]).
One JSON line per scene on stdout (profiles/pcg/ keeps them).
usage: python tools/pcg_time.py [M:N ...]     (default 1000:200000 4000:400000)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bundleadjustmentmatlab_amd as pkg  # noqa: E402
from bundleadjustmentmatlab_amd.scene import make_config  # noqa: E402

VARIANTS = (("auto", {}), ("pcg-0.1", dict(solver="pcg", pcg_tol=0.1)),
            ("pcg-1e-6", dict(solver="pcg", pcg_tol=1e-6, pcg_max_iter=2000)))
ROUNDS, PASSES = 3, 5


def main():
    for spec in sys.argv[1:] or ["1000:200000", "4000:400000"]:
        m, n = (int(v) for v in spec.split(":"))
        sc = make_config("ladybug", m=m, n=n)
        a0 = np.vstack([sc.w0, sc.T0])
        b0 = np.asfortranarray(sc.X0[:3])
        args = (sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6)
        ctx = {name: pkg.BundleAdjuster(*args, **kw) for name, kw in VARIANTS}
        out = dict(scene=f"ladybug m={m} n={n}", observations=int(sc.num_obs), variants={})
        ms = {name: [] for name in ctx}
        its = {name: [] for name in ctx}
        for ba in ctx.values():
            ba.set_params(a0, b0)
            for _ in range(2):                      # warm-up
                ba.step(relinearize=True, update_lm=False)
            ba.sync()
        for _ in range(ROUNDS):                     # alternating: drift hits every variant alike
            for name, ba in ctx.items():
                t0 = time.perf_counter()
                for _ in range(PASSES):
                    ba.step(relinearize=True, update_lm=False)
                ba.sync()
                ms[name].append(1e3 * (time.perf_counter() - t0) / PASSES)
                if name != "auto":
                    its[name].append(ba.pcg_stats()["iterations"])
        for name, ba in ctx.items():
            p = ba.plan_info()
            v = dict(pass_ms=[round(x, 3) for x in ms[name]], solve_bytes=p["solve_bytes"],
                     cr_levels=p["cr_levels"], nd_arcs=p["nd_arcs"], tiles=p["tiles"])
            if name != "auto":
                v["iterations_per_pass"] = its[name]
            out["variants"][name] = v
            ba.close()
        # whole runs (the reference's rule, stop_rel 1e-9): auto against the default tolerance
        for name, kw in (VARIANTS[0], VARIANTS[1]):
            with pkg.BundleAdjuster(*args, stop_rel=1e-9, max_iter=30, **kw) as ba:
                ba.set_params(a0, b0)
                ba.sync()
                t0 = time.perf_counter()
                err, st = ba.run()
                dt = time.perf_counter() - t0
                v = out["variants"][name]
                v.update(run_s=round(dt, 4), run_passes=int(st.iterations),
                         run_final_cost=float(err[-1]))
                if name != "auto":
                    v["run_cg_iterations"] = ba.pcg_stats()["total"]
        f0 = out["variants"]["auto"]["run_final_cost"]
        out["run_final_cost_rel_diff"] = abs(out["variants"]["pcg-0.1"]["run_final_cost"] - f0) / f0
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
