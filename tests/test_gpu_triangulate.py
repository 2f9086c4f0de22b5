"""GPU: vlgba_triangulate (bundle.triangulate_points) against the CPU
references of tests/triang_ref.py, and the growing driver's
``triangulation="gpu"`` switch.

Accuracy bar (set by the issue): max_i ||X_gpu - X_mp|| / ||X_mp|| over the
batch at most 16 x the same maximum of numpy's SVD restatement on the same
batch -- the attainable error is eps x the conditioning of the smallest
singular vector, which is the scene's, not the kernel's.

Shape tests compare with the SVD restatement to 1e-9 relative on the batch
maximum: both sides are within ~1e-12 of the exact solution on these scenes
(the accuracy test measures it), while a lane that read a neighbour's rows, a
wrong camera or a wrong view count moves X by the scene's noise level or more
(>= 1e-4 relative), so 1e-9 separates the two with decades on either side."""
import numpy as np
import pytest

import triang_ref as tr

pytestmark = pytest.mark.gpu


def _scene(**kw):
    from bundleadjustmentmatlab_amd.scene import make_config
    return make_config("cfg1", **kw)


@pytest.fixture(scope="module")
def accuracy_cases():
    """cfg1 (m 6, 30..40 points, seed 4), noisy observations: every point from
    its first 2, 3 and 6 views -- one CSR batch per k with its SVD and 60-digit
    references (computed once)."""
    sc = _scene(m=6, min_n=30, max_n=40, seed=4)
    cnt = np.bincount(sc.obs_pt, minlength=sc.n)
    out = []
    for k in (2, 3, 6):
        pts = np.nonzero(cnt >= k)[0]
        csr = tr.tracks(sc, pts=pts, first=k)
        Xs, st = tr.triangulate_ref(sc.K, sc.T, sc.w, *csr)
        Xm = tr.triangulate_mp(sc.K, sc.T, sc.w, *csr)
        assert np.all(st == 1)
        out.append((k, csr, Xs, Xm))
    assert sum(len(c[1][0]) - 1 for c in out) == 112
    return sc, out


def test_accuracy_against_60_digit_reference(gpu, accuracy_cases):
    sc, cases = accuracy_cases
    for k, csr, Xs, Xm in cases:
        X, st = gpu.triangulate_points(sc.K, sc.T, sc.w, *csr, return_status=True)
        assert np.all(st == 1) and np.all(X[3] == 1.0)
        e_gpu, e_svd = tr.rel_err(X, Xm), tr.rel_err(Xs, Xm)
        print(f"k={k}: {X.shape[1]} points  gpu {e_gpu:.3e}  numpy svd {e_svd:.3e}  "
              f"ratio {e_gpu / e_svd:.3f}")
        assert e_gpu <= 16 * e_svd, (k, e_gpu, e_svd)


@pytest.fixture(scope="module")
def big():
    """291 points in 6 cameras, 257 of them in every camera"""
    sc = _scene(m=6, min_n=260, max_n=300, seed=4)
    pts = np.nonzero(np.bincount(sc.obs_pt, minlength=sc.n) >= 2)[0]
    assert len(pts) >= 257
    return sc, pts


def _check(gpu, sc, csr, K=None, T=None, w=None):
    K, T, w = (sc.K if K is None else K), (sc.T if T is None else T), (sc.w if w is None else w)
    X, st = gpu.triangulate_points(K, T, w, *csr, return_status=True)
    Xr, sr = tr.triangulate_ref(K, T, w, *csr)
    assert np.array_equal(st, sr)
    ok = sr == 1
    assert np.all(X[:, ~ok] == 0.0) and np.all(X[3, ok] == 1.0)
    if ok.any():
        assert tr.rel_err(X[:, ok], Xr[:, ok]) <= 1e-9
    return X, st


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 257])
def test_batch_sizes_at_wave_edges(gpu, big, nb):
    """one lane per point, a wave per workgroup: whole waves, a last wave
    partly empty, one lane alone; mixed track lengths in the batch"""
    sc, pts = big
    X, st = _check(gpu, sc, tr.tracks(sc, pts=pts[-nb:]))
    assert X.shape == (4, nb) and np.all(st == 1)


def test_two_views_in_descending_camera_order(gpu, big):
    sc, pts = big
    csr = tr.tracks(sc, pts=pts[:70], first=2, descending=True)
    assert np.all(np.diff(csr[0]) == 2) and np.all(csr[1][0::2] > csr[1][1::2])
    _check(gpu, sc, csr)


def test_camera_mask_drops_cameras(gpu, big):
    sc, pts = big
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    csr = tr.tracks(sc, mask, pts=pts[:100])
    assert not np.isin(csr[1], [1, 4]).any()
    _check(gpu, sc, csr)


def test_long_track_beside_short_ones(gpu):
    """one planted track of >= 40 views on a 48-camera scene: one long lane in
    a wave of short ones"""
    from bundleadjustmentmatlab_amd.scene import project
    sc = _scene(m=48, min_n=30, max_n=40, seed=4)
    cl, xl = tr.unpack(*tr.tracks(sc, pts=np.arange(1, 31), first=3))
    cams = np.arange(sc.m, dtype=np.int32)
    xt, depth = project(sc.K, sc.w, sc.T, sc.X, cams, np.zeros(sc.m, dtype=int))
    cams = cams[depth > 0][:44]
    assert len(cams) >= 40
    noise = 0.5 * np.random.default_rng(1).standard_normal((len(cams), 2))
    cl.insert(10, cams)                              # the planted track: point 0
    xl.insert(10, xt[cams] + noise)
    ptr, cam, x = tr.pack(cl, xl)
    assert ptr[11] - ptr[10] >= 40 and np.all(np.delete(np.diff(ptr), 10) <= 3)
    X, st = _check(gpu, sc, (ptr, cam, x))
    assert st[10] == 1
    assert np.allclose(X[:3, 10], sc.X[:3, 0], rtol=1e-2, atol=1e-2 * 100)


def test_points_with_one_view_and_none(gpu, big):
    sc, pts = big
    cl, xl = tr.unpack(*tr.tracks(sc, pts=pts[:5]))
    cl += [np.array([2]), np.zeros(0, dtype=int)]               # one view, then none
    xl += [np.array([[250.0, 250.0]]), np.zeros((0, 2))]
    X, st = _check(gpu, sc, tr.pack(cl, xl))
    assert list(st) == [1] * 5 + [2, 2] and np.all(X[:, 5:] == 0.0)


def test_depth_test_rejects_the_restatements_set(gpu):
    """One camera moved so that it sees points at negative depth, as
    test_evaluation.py::test_triangulation_restatement moves it (T_z set so
    that the first point lies 5 behind the camera; negating T alone rejects
    nothing on these scenes, |T| being a few units against a depth of 100),
    the observations re-projected (noise-free) in the moved cameras: exactly
    the points the restatement rejects are rejected.
    Precondition, asserted on the CPU reference: every view's |P3 X| is at
    least 1e-6 of the scene depth (100), so a rounding-size difference cannot
    flip a sign."""
    import copy
    from bundleadjustmentmatlab_amd.evaluation import vl_rodr
    from bundleadjustmentmatlab_amd.scene import project
    sc = copy.copy(_scene(m=6, min_n=60, max_n=80, seed=11))
    j = 2
    i = sc.obs_pt[sc.obs_cam == j][0]
    T2 = sc.T.copy()
    T2[2, j] = -(vl_rodr(sc.w[:, j]) @ sc.X[:3, i])[2] - 5.0
    xt, _ = project(sc.K, sc.w, T2, sc.X, sc.obs_cam, sc.obs_pt)
    sc.obs_x = np.ascontiguousarray(xt)
    pts = np.nonzero(np.bincount(sc.obs_pt, minlength=sc.n) >= 2)[0]
    csr = tr.tracks(sc, pts=pts)
    Xr, sr, depths = tr.triangulate_ref(sc.K, T2, sc.w, *csr, return_depth=True)
    assert min(np.abs(d).min() for d in depths) >= 1e-6 * 100.0
    assert (sr == 0).any() and (sr == 1).any()
    X, st = _check(gpu, sc, csr, T=T2)
    assert np.array_equal(st == 0, sr == 0)


def test_driver_switch(gpu):
    """incremental_bundle(triangulation="gpu") on the reduced growing scene of
    test_gpu_incremental.py: the same cameras and reconstructed set as "host",
    the last solve's final error_ within 1e-4 relative (the direct-difference
    bar for reduced scenes); "host" equals a run without the argument bit for
    bit."""
    from bundleadjustmentmatlab_amd import incremental as inc
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg5", m=10, seed=5)
    dflt = inc.incremental_bundle(sc)
    host = inc.incremental_bundle(sc, triangulation="host")
    dev = inc.incremental_bundle(sc, triangulation="gpu")
    for k in ("K", "T", "w", "X", "status"):
        assert np.array_equal(dflt[k], host[k]), k
    for p, q in zip(dflt["solves"], host["solves"]):
        assert np.array_equal(p["error"], q["error"])
    assert np.array_equal(dev["status"], host["status"])
    assert np.array_equal(dev["X"][3] == 1, host["X"][3] == 1)
    assert len(dev["solves"]) == len(host["solves"])
    e_d, e_h = dev["solves"][-1]["error"][-1], host["solves"][-1]["error"][-1]
    print(f"final error_: gpu {e_d:.12g} host {e_h:.12g} rel {abs(e_d - e_h) / e_h:.3e}")
    assert abs(e_d - e_h) <= 1e-4 * e_h
    with pytest.raises(ValueError):
        inc.incremental_bundle(sc, triangulation="device")
