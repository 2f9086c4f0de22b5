"""Device time of vlgba_covariance on a named config (default cfg3): after a
warm-up (three relinearising passes and three calls), the median over 20 calls
of the camera stage (info[4]; dense method: undamped Schur phase, dense
assembly, dpotrf, dpotri, mirror; selected method: Schur phase, tile assembly,
the cyclic reduction's factor launches, the descent and the extraction) and of
the point kernel (info[5]: k_point_cov), the kernel's algorithmic bytes -- W (N
num_a 3 doubles), V+ and the output (n 9 doubles each) and the co-visible blocks
of Sigma_a (j >= k, num_a^2 doubles each) -- and the rate they imply against
the measured stream rate (profiles/r06/ubench_stream.txt: 6.15 TB/s).
--method dense (default) | selected | both.  both: the two methods alternate
call by call on one context (one box, one state), each with its median, min,
max and scratch, and the largest per-block relative difference between their
diagonal blocks.
usage: python tools/cov_time.py [--method M] [config ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bundleadjustmentmatlab_amd as pkg  # noqa: E402
from bundleadjustmentmatlab_amd.scene import make_config  # noqa: E402

STREAM_TBS = 6.15
CALLS = 20
STAGE = {"dense": "dense inverse (Schur + assemble + dpotrf + dpotri + mirror)",
         "selected": "selected inverse (Schur + assemble + factor + descent + extraction)"}

args = sys.argv[1:]
method = "dense"
if "--method" in args:
    k = args.index("--method")
    method = args[k + 1]
    del args[k:k + 2]
if method not in ("dense", "selected", "both"):
    sys.exit(__doc__)
methods = ["dense", "selected"] if method == "both" else [method]

for name in args or ["cfg3"]:
    sc = make_config(name)
    a0 = np.vstack([sc.w0, sc.T0])
    b0 = np.asfortranarray(sc.X0[:3])
    pivot = np.arange(sc.m) < 2
    with pkg.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, pivot=pivot) as ba:
        ba.set_params(a0, b0)
        for _ in range(3):
            ba.step(relinearize=True, update_lm=False)
        info = np.zeros(8)
        ms = {k: [] for k in methods}
        scratch = {}
        for q in range(3 + CALLS):
            for k in methods:   # alternated call by call
                ba.set_covariance_method(k)
                pkg._lib.check(ba._L.vlgba_covariance(ba._h, 0, None, None, None,
                                                      pkg.bundle._dp(info)), "vlgba_covariance")
                scratch[k] = info[6]
                if q >= 3:
                    ms[k].append((info[4], info[5]))
        cam = {k: ba.covariance(scale=False, method=k)["cam"] for k in methods}
        plan = ba.plan_info()
    N, n, na = plan["obs"], plan["points"], plan["num_a"]
    nbytes = 8 * (N * na * 3 + 2 * 9 * n + plan["blocks"] * na * na)
    track = np.bincount(sc.obs_pt, minlength=sc.n)
    pairs = int((track * (track + 1) // 2).sum())
    print(f"{name}: m {sc.m} n {n} obs {N} num_a {na} ld {na * sc.m} pairs (j >= k) {pairs} "
          f"cyclic-reduction levels {plan['cr_levels']} rows {plan['cr_rows']}")
    for k in methods:
        t = np.array(ms[k])
        stage, pts = np.median(t, axis=0)
        rate = nbytes / (pts * 1e-3) / 1e12
        print(f"  {STAGE[k]}: {stage:.3f} ms median of {CALLS} (min {t[:, 0].min():.3f}, max "
              f"{t[:, 0].max():.3f}), scratch {scratch[k] / 1e6:.1f} MB ({int(scratch[k])} bytes)")
        print(f"  k_point_cov: {1e3 * pts:.1f} us median of {CALLS} (min "
              f"{1e3 * t[:, 1].min():.1f}, max {1e3 * t[:, 1].max():.1f}); algorithmic bytes "
              f"{nbytes / 1e6:.1f} MB -> {rate:.3f} TB/s = {rate / STREAM_TBS:.3f} of the "
              f"{STREAM_TBS} TB/s stream rate", flush=True)
    if len(methods) == 2:
        d = np.abs(cam["selected"] - cam["dense"]).max(axis=(0, 1))
        r = np.abs(cam["dense"]).max(axis=(0, 1))
        fig = np.where(r > 0, d / np.where(r > 0, r, 1), np.where(d > 0, np.inf, 0)).max()
        print(f"  selected against dense, diagonal blocks: largest per-block max|diff| / "
              f"max|dense block| {fig:.3g}", flush=True)
