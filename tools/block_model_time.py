#!/usr/bin/env python3
"""Timing of the batched one-camera / one-point entries and their modes
(profiles/block_model/): vlgba_resect, vlgba_intersect, vlgba_triangulate and
vlgba_resect_ex, vlgba_intersect_ex, vlgba_triangulate_ex on the batches of the
existing large tests --

  resect     the 1000 cameras of config 3 (~3000 observations each) against the
             true structure (tests/test_gpu_resect.py::test_resect_batch_large)
  intersect  20 000 six-view points of config 2's model at m = 50, started 0.05
             off (tests/test_gpu_intersect.py::test_batch_of_20000_points)

-- with, optionally, an older build of the library beside the package's own
(--parent PATH: its plain entries are timed in the same process, interleaved
with this build's, so that both see the same machine state).

Every figure is the wall time of one whole call on host pointers (uploads, every
LM pass, downloads; the call ends in a stream synchronise), in ms: the median of
--reps calls after --warmup calls, with the smallest and largest beside it; the
variants of a group are called in turn within each repetition.  One JSON line
per variant on stdout; "outputs" is a hash of everything the call returned
(parameters, error_, counts / status), so equal hashes mean equal bits.  Radial
variants run on the same geometry observed through the lens radial_ref.K_TRUE."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, ROOT)
K_TRUE = (-0.15, 0.03)


def digest(*arrays):
    """a short hash of the call's outputs: equal digests, equal bits"""
    h = hashlib.sha256()
    for q in arrays:
        h.update(np.ascontiguousarray(q).tobytes())
    return h.hexdigest()[:16]


def valid(err, nerr):
    """error_ rows with the entries past each row's count zeroed"""
    return np.where(np.arange(err.shape[1])[None, :] < nerr[:, None], err, 0.0)


def timed(call):
    """(return code, ms) of one library call"""
    t0 = time.perf_counter()
    rc = call()
    return rc, (time.perf_counter() - t0) * 1e3


def distort(K, x, cam):
    """the pinhole pixels x (N, 2) of cameras cam seen through the lens K_TRUE
    (f = K[0]): x = f d n + c with n = (x - c) / f"""
    f, c = K[0, cam][:, None], K[2:4, cam].T
    n = (x - c) / f
    r2 = (n * n).sum(1)[:, None]
    return f * ((1 + K_TRUE[0] * r2 + K_TRUE[1] * r2 * r2) * n) + c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", help="an older libvlgba.so to time beside this build")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=0, help="resect: the first N cameras (0: all)")
    ap.add_argument("--points", type=int, default=20_000)
    ap.add_argument("--groups", default="resect,intersect,triangulate")
    a = ap.parse_args()

    import bundleadjustmentmatlab_amd as pkg
    from bundleadjustmentmatlab_amd import _lib
    from bundleadjustmentmatlab_amd._lib import (VlgbaOptions, VlgbaResectProblem, VlgbaStats,
                                                 c_dp, c_ip)
    from bundleadjustmentmatlab_amd.scene import make_config
    new = pkg.lib()
    old = None
    if a.parent:
        old = ctypes.CDLL(a.parent)
        for nm in ("vlgba_resect", "vlgba_intersect", "vlgba_triangulate"):
            getattr(old, nm).restype, getattr(old, nm).argtypes = _lib.SIGNATURES[nm]
    llp = ctypes.POINTER(ctypes.c_longlong)
    dp = lambda x: x.ctypes.data_as(c_dp)
    opt = VlgbaOptions()

    def measure(group, variants):
        """variants: [(name, fn)], fn() -> (ms of the library call, figures of
        merit); called in turn"""
        times = {nm: [] for nm, _ in variants}
        merit = {}
        for r in range(a.warmup + a.reps):
            for nm, fn in variants:
                dt, merit[nm] = fn()
                if r >= a.warmup:
                    times[nm].append(dt)
        for nm, _ in variants:
            t = times[nm]
            print(json.dumps(dict(group=group, variant=nm, median_ms=round(statistics.median(t), 3),
                                  min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=len(t),
                                  **merit[nm])), flush=True)

    groups = a.groups.split(",")
    if "resect" in groups:
        sc = make_config("cfg3")
        order = np.argsort(sc.obs_cam, kind="stable")
        cam, pt = sc.obs_cam[order], sc.obs_pt[order]
        m = a.cameras or sc.m
        ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=sc.m))]).astype(np.int64)
        ptr = np.ascontiguousarray(ptr[:m + 1])
        N = int(ptr[-1])
        X = np.ascontiguousarray(sc.X[:3, pt[:N]].T)
        x = np.ascontiguousarray(sc.obs_x[order][:N])
        xr = np.ascontiguousarray(distort(sc.K, x, cam[:N]))
        K = np.ascontiguousarray(sc.K[:, :m].T)
        a6 = np.ascontiguousarray(np.vstack([sc.w0[:, :m], sc.T0[:, :m]]).T)
        a9 = np.ascontiguousarray(np.hstack([a6, K[:, :1], np.zeros((m, 2))]))   # k1 = k2 = 0
        cap = 21
        err = np.zeros((m, cap))
        nerr = np.zeros(m, dtype=np.int32)

        def resect(L, ex, na, a0, xo, jac=0, loss=0, scale=0.0):
            pr = VlgbaResectProblem(m, na, ptr.ctypes.data_as(llp), dp(X), dp(xo), dp(K))

            def fn():
                av = a0.copy()
                st = VlgbaStats()
                if ex:
                    rc, dt = timed(lambda: L.vlgba_resect_ex(
                        ctypes.byref(pr), ctypes.byref(opt), jac, loss, scale, dp(av), dp(err), cap,
                        nerr.ctypes.data_as(c_ip), None, None, ctypes.byref(st)))
                else:
                    rc, dt = timed(lambda: L.vlgba_resect(
                        ctypes.byref(pr), ctypes.byref(opt), dp(av), dp(err), cap,
                        nerr.ctypes.data_as(c_ip), ctypes.byref(st)))
                assert rc == 0, rc
                last = err[np.arange(m), nerr - 1]
                return dt, dict(passes=st.iterations, accepted=st.accepted,
                                worst_final_error=float(last.max()), observations=N, cameras=m,
                                outputs=digest(av, valid(err, nerr), nerr))
            return fn
        v = [("vlgba_resect", resect(new, False, 6, a6, x)),
             ("resect_ex fd none", resect(new, True, 6, a6, x)),
             ("resect_ex analytic none", resect(new, True, 6, a6, x, jac=1)),
             ("resect_ex fd huber 3", resect(new, True, 6, a6, x, loss=1, scale=3.0)),
             ("resect_ex fd cauchy 3", resect(new, True, 6, a6, x, loss=2, scale=3.0)),
             ("resect_ex analytic huber 3", resect(new, True, 6, a6, x, jac=1, loss=1, scale=3.0)),
             ("resect_ex radial", resect(new, True, 9, a9, xr, jac=1))]
        if old is not None:
            v.insert(0, ("parent vlgba_resect", resect(old, False, 6, a6, x)))
        measure("resect", v)

    if "intersect" in groups or "triangulate" in groups:
        sc = make_config("cfg2", m=50, n=a.points, track=6, seed=9)
        n = sc.n
        ptr = np.searchsorted(sc.obs_pt, np.arange(n + 1)).astype(np.int64)
        cam = np.ascontiguousarray(sc.obs_cam, dtype=np.int32)
        x = np.ascontiguousarray(sc.obs_x, dtype=np.float64)
        xr = np.ascontiguousarray(distort(sc.K, x, cam))
        K, T, w = (np.ascontiguousarray(q.T) for q in (sc.K, sc.T, sc.w))
        Kf = K.copy()
        Kf[:, 1] = Kf[:, 0]
        kd = np.ascontiguousarray(np.tile(K_TRUE, (sc.m, 1)))
        kd0 = np.zeros_like(kd)
        X0 = np.ascontiguousarray((sc.X[:3] + 0.05).T)
        cap = 21
        err = np.zeros((n, cap))
        nerr = np.zeros(n, dtype=np.int32)
        head = lambda Kq: (sc.m, dp(Kq), dp(T), dp(w))
        tail = lambda xo: (n, ptr.ctypes.data_as(llp), cam.ctypes.data_as(c_ip), dp(xo))

        def isect(L, ex, Kq=K, kdq=None, xo=x, jac=0, loss=0, scale=0.0):
            def fn():
                b = X0.copy()
                st = VlgbaStats()
                if ex:
                    rc, dt = timed(lambda: L.vlgba_intersect_ex(
                        *head(Kq), None if kdq is None else dp(kdq), *tail(xo), ctypes.byref(opt),
                        jac, loss, scale, dp(b), dp(err), cap, nerr.ctypes.data_as(c_ip), None,
                        None, ctypes.byref(st)))
                else:
                    rc, dt = timed(lambda: L.vlgba_intersect(
                        *head(Kq), *tail(xo), ctypes.byref(opt), dp(b), dp(err), cap,
                        nerr.ctypes.data_as(c_ip), ctypes.byref(st)))
                assert rc == 0, rc
                last = err[np.arange(n), np.maximum(nerr, 1) - 1]
                return dt, dict(passes=st.iterations, accepted=st.accepted,
                                mean_final_error=float(last.mean()), points=n,
                                observations=int(ptr[-1]), outputs=digest(b, valid(err, nerr), nerr))
            return fn

        def tri(L, ex, Kq=K, kdq=None, xo=x):
            Xo = np.zeros((n, 4))
            stt = np.zeros(n, dtype=np.int32)

            def fn():
                if ex:
                    rc, dt = timed(lambda: L.vlgba_triangulate_ex(
                        *head(Kq), None if kdq is None else dp(kdq), *tail(xo), 0, dp(Xo),
                        stt.ctypes.data_as(c_ip)))
                else:
                    rc, dt = timed(lambda: L.vlgba_triangulate(
                        *head(Kq), *tail(xo), 0, dp(Xo), stt.ctypes.data_as(c_ip)))
                assert rc == 0, rc
                ok = stt == 1
                worst = float(np.abs(Xo[ok, :3] - sc.X[:3].T[ok]).max()) if ok.any() else None
                return dt, dict(triangulated=int(ok.sum()), points=n, worst_error=worst,
                                outputs=digest(Xo, stt))
            return fn
        if "intersect" in groups:
            v = [("vlgba_intersect", isect(new, False)),
                 ("intersect_ex fd none", isect(new, True)),
                 ("intersect_ex analytic none", isect(new, True, jac=1)),
                 ("intersect_ex fd huber 3", isect(new, True, loss=1, scale=3.0)),
                 ("intersect_ex fd cauchy 3", isect(new, True, loss=2, scale=3.0)),
                 ("intersect_ex radial", isect(new, True, Kf, kd, xr, jac=1))]
            if old is not None:
                v.insert(0, ("parent vlgba_intersect", isect(old, False)))
            measure("intersect", v)
        if "triangulate" in groups:
            v = [("vlgba_triangulate", tri(new, False)),
                 ("triangulate_ex no lens", tri(new, True)),
                 ("triangulate_ex zero lens", tri(new, True, Kf, kd0, x)),
                 ("triangulate_ex radial", tri(new, True, Kf, kd, xr))]
            if old is not None:
                v.insert(0, ("parent vlgba_triangulate", tri(old, False)))
            measure("triangulate", v)


if __name__ == "__main__":
    main()
