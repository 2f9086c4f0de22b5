#!/usr/bin/env python3
"""k_schur_mfma's chunk loop, wave by wave (diagnostic build).

Build ``make -C bundleadjustmentmatlab_amd/csrc stamps`` (libvlgba_stamps.so,
-DBA_STAMPS), then on the GPU box:  python tools/schur_head_stamps.py [cfg]
(VLGBA_STAMPS_LIB: another stamps build).  Prints
  * the share of an iteration's four phases -- top -> last global load issued
    -> first MFMA issued -> last MFMA issued -> next top -- over every wave;
  * whether the waves that share a SIMD enter their MFMA clusters together:
    for every pair of co-resident waves, the distance of their first-MFMA
    clocks at chunks 8, 16, 24, folded into one chunk period, against the
    length of the MFMA phase.  Waves in random phase overlap their MFMA
    windows in min(1, 2 L / P) of the pairs (L: MFMA phase, P: period).
"""
import ctypes
import os
import sys
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundleadjustmentmatlab_amd._lib as L  # noqa: E402

L.LIB_PATH = os.environ.get("VLGBA_STAMPS_LIB") or os.path.join(
    ROOT, "bundleadjustmentmatlab_amd", "libvlgba_stamps.so")
from bundleadjustmentmatlab_amd import BundleAdjuster  # noqa: E402
from bundleadjustmentmatlab_amd.scene import make_config  # noqa: E402

PHASES = ["top -> loads issued", "-> first MFMA", "-> last MFMA", "-> next top (flush)"]
MAX_WG = 4096


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    sc = make_config(cfg)
    lib = L.lib()
    fn = lib.vlgba_debug_mf_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    a = np.zeros((6, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    ba = BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6)
    ba.set_params(a, b)
    for _ in range(60):   # clocks up; the records are the last launch's
        ba.step(relinearize=True, update_lm=False)
    ba.sync()
    ngrp = min(int(ba.plan_info()["mfma_groups"]), MAX_WG)
    buf = np.zeros(ngrp * 4 * 8, dtype=np.uint64)
    assert fn(buf.ctypes.data, buf.size) == 0
    ba.close()
    rec = buf.reshape(ngrp * 4, 8)
    nch = (rec[:, 4] >> np.uint64(56)).astype(np.int64)
    rec = rec[nch > 0]
    nch = nch[nch > 0]
    ph = rec[:, 0:4].astype(np.float64)
    tot = ph.sum()
    print(f"k_schur_mfma {cfg}: {len(rec)} waves, {nch.sum() // 4} chunks, "
          f"{ph.sum(axis=1).mean():.0f} cycles of chunk loop per wave")
    for i, name in enumerate(PHASES):
        print(f"  {name:22s} {100 * ph[:, i].sum() / tot:5.1f}%  "
              f"{ph[:, i].sum() / nch.sum():8.0f} cycles/chunk")
    period = ph.sum(axis=1) / nch
    lm = ph[:, 2] / nch
    P, Lm = period.mean(), lm.mean()
    print(f"  period P {P:.0f} cycles, MFMA phase L {Lm:.0f} cycles: waves in random phase "
          f"overlap in {100 * min(1.0, 2 * Lm / P):.0f}% of the pairs, mean distance P/4 "
          f"= {P / 4:.0f}")
    hw = rec[:, 4] & np.uint64(0xffffffff)
    xcc = (rec[:, 4] >> np.uint64(32)) & np.uint64(0xf)
    simd = (hw >> np.uint64(4)) & np.uint64(3)
    cu = (hw >> np.uint64(8)) & np.uint64(0xf)
    sh = (hw >> np.uint64(12)) & np.uint64(1)
    se = (hw >> np.uint64(13)) & np.uint64(7)
    groups = defaultdict(list)
    for q in range(len(rec)):
        groups[(int(xcc[q]), int(se[q]), int(sh[q]), int(cu[q]), int(simd[q]))].append(q)
    sizes = np.bincount([len(v) for v in groups.values()])
    print(f"  {len(groups)} SIMDs hold waves; waves per SIMD: "
          + ", ".join(f"{n} x {c}" for n, c in enumerate(sizes) if c))
    for j, k in enumerate((8, 16, 24)):
        d = []
        for v in groups.values():
            for x in range(len(v)):
                for y in range(x + 1, len(v)):
                    tx, ty = int(rec[v[x], 5 + j]), int(rec[v[y], 5 + j])
                    if tx == 0 or ty == 0:
                        continue
                    p = 0.5 * (period[v[x]] + period[v[y]])
                    r = abs(tx - ty) % p
                    d.append((min(r, p - r), abs(tx - ty)))
        if not d:
            continue
        d = np.array(d)
        q = np.percentile(d[:, 0], [10, 25, 50, 75, 90])
        print(f"  chunk {k:2d}: {len(d)} pairs; folded distance of first MFMAs: mean "
              f"{d[:, 0].mean():.0f}, p10/25/50/75/90 " + "/".join(f"{x:.0f}" for x in q)
              + f"; closer than L: {100 * np.mean(d[:, 0] < Lm):.0f}%; closer than L/4: "
              f"{100 * np.mean(d[:, 0] < Lm / 4):.0f}% (random: "
              f"{100 * min(1.0, Lm / 2 / P):.0f}%); raw |dt| median {np.median(d[:, 1]):.0f}")


if __name__ == "__main__":
    main()
