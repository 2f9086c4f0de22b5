"""CPU: the references of the batched per-point entries (tests/triang_ref.py)
and the parts of vlgba_triangulate / vlgba_intersect that need no GPU: the
header, the binding and the argument checks.

Tolerances.  Noise-free observations: the true points to 1e-7 (absolute and
relative), the bar of test_evaluation.py::test_triangulation_restatement.  The
60-digit reference against numpy's SVD: 1e-10 relative on the batch maximum --
the SVD's own error on these scenes is eps x the conditioning of the smallest
singular vector, at most ~1e-12 (the issue's measurement: max 8.5e-13), so
1e-10 leaves two decades and still catches a wrong vector (O(1))."""
import ctypes
import os
import re

import numpy as np
import pytest

import triang_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    from bundleadjustmentmatlab_amd.scene import make_config
    return make_config("cfg1", m=6, min_n=30, max_n=40, seed=4)


def test_restatement_equals_driver_triangulate(scene):
    """triang_ref.triangulate_ref (one SVD per point) equals the growing
    driver's vectorised ``_triangulate`` bit for bit.  ``_triangulate`` pads a
    batch's systems with zero rows to the longest track, which changes the path
    LAPACK takes for a short one, so the driver is called on the points of one
    track length at a time (no padding); every track length of the scene is
    covered, and a camera mask."""
    from bundleadjustmentmatlab_amd import incremental as inc
    sc = scene
    for mask in (np.ones(sc.m, dtype=bool), np.array([1, 0, 1, 1, 0, 1], dtype=bool)):
        cnt = np.bincount(sc.obs_pt, weights=mask[sc.obs_cam], minlength=sc.n).astype(int)
        lengths = [k for k in np.unique(cnt) if k >= 2]
        assert len(lengths) >= 2
        for k in lengths:
            pts = np.nonzero(cnt == k)[0]
            X = inc._triangulate(sc, sc.K, sc.T, sc.w, pts, mask)
            Xr, st = tr.triangulate_ref(sc.K, sc.T, sc.w, *tr.tracks(sc, mask, pts))
            assert np.array_equal(X, Xr), k
            assert np.array_equal(st == 1, X[3] == 1.0)


def test_noise_free_observations_recover_the_points(scene):
    import copy
    from bundleadjustmentmatlab_amd.scene import project
    sc = copy.copy(scene)
    xt, _ = project(sc.K, sc.w, sc.T, sc.X, sc.obs_cam, sc.obs_pt)
    sc.obs_x = np.ascontiguousarray(xt)
    ptr, cam, x = tr.tracks(sc)
    X, st = tr.triangulate_ref(sc.K, sc.T, sc.w, ptr, cam, x)
    assert np.all(st == 1) and np.all(X[3] == 1.0)
    assert np.allclose(X[:3], sc.X[:3], rtol=1e-7, atol=1e-7)
    Xm = tr.triangulate_mp(sc.K, sc.T, sc.w, ptr[:6], cam, x)
    assert np.allclose(Xm[:3], sc.X[:3, :5], rtol=1e-7, atol=1e-7)


def test_mpmath_and_numpy_references_agree(scene):
    sc = scene
    cnt = np.bincount(sc.obs_pt, minlength=sc.n)
    for k in (2, 6):
        pts = np.nonzero(cnt >= k)[0][:12]
        ptr, cam, x = tr.tracks(sc, pts=pts, first=k)
        X, st = tr.triangulate_ref(sc.K, sc.T, sc.w, ptr, cam, x)
        Xm = tr.triangulate_mp(sc.K, sc.T, sc.w, ptr, cam, x)
        assert np.all(st == 1)
        assert np.all(Xm[3] == 1.0)
        assert tr.rel_err(X, Xm) <= 1e-10


def test_tracks_helper(scene):
    sc = scene
    mask = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    ptr, cam, x = tr.tracks(sc, mask, pts=[3, 0], first=3, descending=True)
    assert ptr.dtype == np.int64 and cam.dtype == np.int32 and x.shape == (ptr[-1], 2)
    for q, i in enumerate((3, 0)):
        ids = np.nonzero((sc.obs_pt == i) & mask[sc.obs_cam])[0][:3][::-1]
        assert np.array_equal(cam[ptr[q]:ptr[q + 1]], sc.obs_cam[ids])
        assert np.array_equal(x[ptr[q]:ptr[q + 1]], sc.obs_x[ids])
        assert np.all(np.diff(cam[ptr[q]:ptr[q + 1]]) < 0)


def test_header_and_binding_declare_both_entries():
    """include/vlgba.h declares vlgba_triangulate and vlgba_intersect, the
    binding mirrors them, the library exports them, and the ABI is still 6."""
    from bundleadjustmentmatlab_amd import _lib
    import bundleadjustmentmatlab_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "vlgba.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(vlgba_\w+)\s*\(", src))
    for nm in ("vlgba_triangulate", "vlgba_intersect"):
        assert nm in names and nm in _lib.SIGNATURES
        assert hasattr(pkg.lib(), nm)
    assert "#define VLGBA_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6
    assert callable(pkg.triangulate_points) and callable(pkg.bundle_euclid_intersect)


def _args(m=2, n=2, ptr=(0, 2, 4), cam=(0, 1, 1, 0)):
    K = np.tile([500.0, 500.0, 250.0, 250.0], m)
    T = np.zeros(3 * m)
    w = np.zeros(3 * m)
    ptr = np.asarray(ptr, dtype=np.int64)
    cam = np.asarray(cam, dtype=np.int32)
    x = np.zeros(2 * len(cam))
    return dict(m=m, K=K, T=T, w=w, n=n, ptr=ptr, cam=cam, x=x)


def _call(which, a, X="own", null=()):
    """call entry ``which`` with the arguments of ``a`` (names in ``null``
    passed as NULL); returns the code"""
    import bundleadjustmentmatlab_amd as pkg
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, c_dp, c_ip
    L = pkg.lib()
    llp = ctypes.POINTER(ctypes.c_longlong)
    p = {k: (None if k in null else
             a[k].ctypes.data_as(llp if k == "ptr" else c_ip if k == "cam" else c_dp))
         for k in ("K", "T", "w", "ptr", "cam", "x")}
    rows = 4 if which == "triangulate" else 3
    Xb = np.zeros(rows * max(a["n"], 1))
    Xp = None if "X" in null else Xb.ctypes.data_as(c_dp)
    if which == "triangulate":
        return L.vlgba_triangulate(a["m"], p["K"], p["T"], p["w"], a["n"], p["ptr"], p["cam"],
                                   p["x"], 0, Xp, None)
    opt = VlgbaOptions()
    return L.vlgba_intersect(a["m"], p["K"], p["T"], p["w"], a["n"], p["ptr"], p["cam"], p["x"],
                             ctypes.byref(opt), Xp, None, 0, None, None)


@pytest.mark.parametrize("which", ["triangulate", "intersect"])
def test_bad_arguments_rejected_before_device_work(which):
    """Every argument error returns VLGBA_E_ARG without touching a device (this
    test runs on a machine without one), and n == 0 succeeds without a launch."""
    E_ARG = -1001
    for nm in ("K", "T", "w", "ptr", "cam", "x", "X"):
        assert _call(which, _args(), null=(nm,)) == E_ARG, nm
    assert _call(which, dict(_args(), m=0)) == E_ARG
    assert _call(which, dict(_args(), n=-1)) == E_ARG
    assert _call(which, _args(ptr=(0, 3, 2))) == E_ARG            # non-monotone
    assert _call(which, _args(ptr=(1, 2, 4))) == E_ARG            # obs_ptr[0] != 0
    assert _call(which, _args(cam=(0, 1, 2, 0))) == E_ARG         # camera id == m
    assert _call(which, _args(cam=(0, -1, 1, 0))) == E_ARG        # negative camera id
    assert _call(which, _args(n=0, ptr=(0,), cam=())) == 0
    # n == 0 needs no track arrays beyond obs_ptr
    assert _call(which, _args(n=0, ptr=(0,), cam=()), null=("cam", "x")) == 0


def test_python_mirrors_with_no_points():
    import bundleadjustmentmatlab_amd as pkg
    K = np.tile([[500.0], [500.0], [250.0], [250.0]], (1, 2))
    z = np.zeros((3, 2))
    X = pkg.triangulate_points(K, z, z, [0], [], np.zeros((0, 2)))
    assert X.shape == (4, 0)
    X_, errs = pkg.bundle_euclid_intersect(K, z, z, np.zeros((3, 0)), [0], [], np.zeros((0, 2)))
    assert X_.shape == (3, 0) and errs == []
