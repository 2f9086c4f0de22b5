"""Device time of vlgba_covariance on a named config (default cfg3): after a
warm-up (three relinearising passes and three calls), the median over 20 calls
of the dense inverse (info[4]: undamped Schur phase, dense assembly, dpotrf,
dpotri, mirror) and of the point kernel (info[5]: k_point_cov), the kernel's
algorithmic bytes -- W (N num_a 3 doubles), V+ and the output (n 9 doubles
each) and the co-visible blocks of Sigma_a (j >= k, num_a^2 doubles each) --
and the rate they imply against the measured stream rate
(profiles/r06/ubench_stream.txt: 6.15 TB/s).
usage: python tools/cov_time.py [config ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bundleadjustmentmatlab_amd as pkg  # noqa: E402
from bundleadjustmentmatlab_amd.scene import make_config  # noqa: E402

STREAM_TBS = 6.15
CALLS = 20

for name in sys.argv[1:] or ["cfg3"]:
    sc = make_config(name)
    a0 = np.vstack([sc.w0, sc.T0])
    b0 = np.asfortranarray(sc.X0[:3])
    pivot = np.arange(sc.m) < 2
    with pkg.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, pivot=pivot) as ba:
        ba.set_params(a0, b0)
        for _ in range(3):
            ba.step(relinearize=True, update_lm=False)
        info = np.zeros(8)
        ms = []
        for q in range(3 + CALLS):
            pkg._lib.check(ba._L.vlgba_covariance(ba._h, 0, None, None, None,
                                                  pkg.bundle._dp(info)), "vlgba_covariance")
            if q >= 3:
                ms.append((info[4], info[5]))
        plan = ba.plan_info()
    dense, pts = np.median(np.array(ms), axis=0)
    N, n, na = plan["obs"], plan["points"], plan["num_a"]
    nbytes = 8 * (N * na * 3 + 2 * 9 * n + plan["blocks"] * na * na)
    rate = nbytes / (pts * 1e-3) / 1e12
    track = np.bincount(sc.obs_pt, minlength=sc.n)
    pairs = int((track * (track + 1) // 2).sum())
    print(f"{name}: m {sc.m} n {n} obs {N} num_a {na} ld {na * sc.m} pairs (j >= k) {pairs}")
    print(f"  dense inverse (Schur + assemble + dpotrf + dpotri + mirror): {dense:.3f} ms "
          f"median of {CALLS} (min {min(m[0] for m in ms):.3f}), scratch "
          f"{info[6] / 1e6:.0f} MB")
    print(f"  k_point_cov: {1e3 * pts:.1f} us median of {CALLS} (min "
          f"{1e3 * min(m[1] for m in ms):.1f}); algorithmic bytes {nbytes / 1e6:.1f} MB -> "
          f"{rate:.3f} TB/s = {rate / STREAM_TBS:.3f} of the {STREAM_TBS} TB/s stream rate",
          flush=True)
