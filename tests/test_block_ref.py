"""CPU: the one-block references (tests/block_ref.py) and the parts of
vlgba_resect_ex / vlgba_intersect_ex / vlgba_triangulate_ex that need no GPU:
the header, the binding and the argument checks.

Tolerances.
  normal equations   block_ref's are the named functions' outputs: equal arrays.
  stationarity       under radial_ref.E2E["stop"] (stop_rel 1e-12) the LM ends
                     where the cost no longer falls by 1e-12 relative.  One more
                     Gauss-Newton step dx = H^-1 g would lower the cost by about
                     g'H^-1 g / 2, so at the end g'H^-1 g <= ~1e-11 cost.  The
                     test computes g by long double central differences of the
                     TRUE projection (step 1e-6: truncation ~1e-12 relative) and
                     asserts g'H^-1 g <= 1e-9 cost -- two decades above the stop
                     rule's own level, ten below a step that matters (the start is
                     >= 1e-1 cost away in that measure).
  undistortion       1e-15 relative, as the issue sets.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import block_ref as br
import jac_ref as jr
import radial_ref as rad
import robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = br.LD
STOP = rad.E2E["stop"]


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD))


@pytest.mark.parametrize("na", [6, 7, 10, 9])
def test_camera_block_is_the_references_linearization(na):
    P, _ = br.synth_camera(40, 11, na)
    eo = np.asarray(br.residuals(P)[0], dtype=np.float64)
    args = (P["K"], P["a"], P["b"], P["pt"], P["cam"], eo, 1, P["n"])
    if na == 9:
        want = rad.linearization(*args, fix_structure=True)
        assert _eq(eo, np.asarray(rad.residuals(P["K"], P["a"], P["b"], P["pt"], P["cam"],
                                                P["obs_x"])[0], dtype=np.float64))
    else:
        want = jr.linearization(*args, na, fix_structure=True)
    R = br.linearization(P)
    H, g, Hb, gb = br.block(P, R)
    assert _eq(H, want["U"][:, :, 0]) and _eq(g, want["eA"][:, 0])
    assert _eq(Hb, want["U_b"][:, :, 0]) and _eq(gb, want["eA_b"][:, 0])
    assert not np.any(np.asarray(R["V"])) and not np.any(np.asarray(R["W"]))
    # ... and robust_ref.weighted's on the same rows, which block_lm uses
    Ao, Bo, _, _ = br.jacobians(P)
    W = rr.weighted(1, P["n"], na, P["pt"], P["cam"], Ao, Bo, eo, "none", 1.0, fix_structure=True)
    assert _eq(W["U"][:, :, 0], H) and _eq(W["eA"][:, 0], g)


@pytest.mark.parametrize("radial", [False, True])
def test_point_block_is_the_references_linearization(radial):
    s = br.synth_tracks([4, 2], 5, radial)
    P = br.track_point(s, 0)
    eo = np.asarray(br.residuals(P)[0], dtype=np.float64)
    args = (P["K"], P["a"], P["b"], P["pt"], P["cam"], eo, P["m"], 1)
    want = (rad.linearization(*args, fix_motion=True) if radial
            else jr.linearization(*args, 6, fix_motion=True))
    H, g, Hb, gb = br.block(P, br.linearization(P))
    assert H.shape == (3, 3)
    assert _eq(H, want["V"][:, :, 0]) and _eq(g, want["eB"][:, 0])
    assert _eq(Hb, want["V_b"][:, :, 0]) and _eq(gb, want["eB_b"][:, 0])


def test_robust_block_is_the_weighted_reference():
    """under a loss the radial block is radial_ref.linearization(kind, c); the
    pinhole block's values are robust_ref.weighted's and its bound is no smaller"""
    P, _ = br.synth_camera(60, 12, 9)
    P["obs_x"], out = rr.plant_outliers(P["obs_x"], frac=0.1, seed=3)
    assert out.sum() >= 2
    eo = np.asarray(br.residuals(P)[0], dtype=np.float64)
    want = rad.linearization(P["K"], P["a"], P["b"], P["pt"], P["cam"], eo, 1, P["n"],
                             kind="huber", c=3.0, fix_structure=True)
    R = br.linearization(P, kind="huber", c=3.0)
    assert _eq(R["U"], want["U"]) and _eq(R["U_b"], want["U_b"]) and _eq(R["eA"], want["eA"])
    assert np.all(np.asarray(R["w"])[out] < 1)
    P6, _ = br.synth_camera(60, 12, 6)
    P6["obs_x"], out = rr.plant_outliers(P6["obs_x"], frac=0.1, seed=3)
    eo = np.asarray(br.residuals(P6)[0], dtype=np.float64)
    Ao, Bo, _, _ = br.jacobians(P6)
    W = rr.weighted(1, P6["n"], 6, P6["pt"], P6["cam"], Ao, Bo, eo, "cauchy", 3.0,
                    fix_structure=True)
    R = br.linearization(P6, kind="cauchy", c=3.0)
    assert _eq(R["U"], W["U"]) and _eq(R["eA"], W["eA"]) and _eq(R["cost"], W["cost"])
    assert np.all(np.asarray(R["U_b"]) >= np.asarray(W["U_b"]))


def test_pinhole_residuals_restate_the_true_projection():
    """the kernel-order pinhole residuals agree with jac_ref.project (the true
    projection) within their own bound plus the table rotation's (|w| >= 1e-6)"""
    for na in (6, 7, 10):
        P, _ = br.synth_camera(30, 13, na)
        e, eb = br.residuals(P)
        xt = jr.project(P["K"], P["a"], P["b"], P["pt"], P["cam"], na)
        d = np.abs(e - (P["obs_x"].astype(LD) - xt))
        assert np.all(eb < 1e-10) and np.all(eb > 0)     # some 30 roundings of ~5e3 px z
        assert np.all(d <= eb), float((d / eb).max())


@pytest.mark.parametrize("kind", ["none", "huber", "cauchy"])
def test_fp64_cost_is_within_the_long_double_costs_bound(kind):
    """block_ref.cost_fp64 (the kernels' operations in fp64) against block_ref.cost
    (long double, every rounding bounded): within that bound, every model"""
    for na in (6, 7, 10, 9):
        P, _ = br.synth_camera(70, 14, na)
        P["obs_x"], _ = rr.plant_outliers(P["obs_x"], frac=0.1, seed=na)
        ref, bound = br.cost(P, kind=kind, c=3.0)
        got = br.cost_fp64(P, kind=kind, c=3.0)
        assert 0 < bound < 1e-9 * ref and abs(got - ref) <= bound, (na, got, ref, bound)
    s = br.synth_tracks([9], 15, True)
    P = br.track_point(s, 0)
    ref, bound = br.cost(P, kind=kind, c=3.0)
    assert abs(br.cost_fp64(P, kind=kind, c=3.0) - ref) <= bound


CASES = [(6, "none"), (7, "none"), (10, "none"), (9, "none"), (9, "huber"), (6, "cauchy")]


@pytest.mark.parametrize("na,kind", CASES)
def test_converged_camera_is_a_stationary_point(na, kind):
    P, a_true = br.synth_camera(80, 21 + na, na)
    if kind != "none":
        P["obs_x"], _ = rr.plant_outliers(P["obs_x"], frac=0.05, seed=na)
    x0 = br.free(P)
    x, err = br.block_lm(P, kind, 3.0, **STOP)
    assert len(err) >= 3 and err[-1] < err[0]
    H = np.asarray(br.block(P, br.linearization(P, *br.with_free(P, x), kind, 3.0))[0],
                   dtype=np.float64)
    measure = lambda xx: (lambda g: float(g @ np.linalg.solve(H, g)))(
        np.asarray(br.gradient_cd(P, xx, kind, 3.0), dtype=np.float64) / 2)
    # cost = sum rho, gradient of it = -2 J'W e: g / 2 is the normal equations' eA
    c_end = float(br.true_cost(P, x.astype(LD), kind, 3.0))
    print(f"na {na} {kind}: g'H^-1 g {measure(x):.2e} (start {measure(x0):.2e}), cost {c_end:.4g}")
    assert measure(x0) >= 1e-1 * c_end
    assert measure(x) <= 1e-9 * c_end


@pytest.mark.parametrize("radial", [False, True])
def test_converged_point_is_a_stationary_point(radial):
    s = br.synth_tracks([5], 31, radial)
    P = br.track_point(s, 0)
    x, err = br.block_lm(P, **STOP)
    H = np.asarray(br.block(P, br.linearization(P, *br.with_free(P, x)))[0], dtype=np.float64)
    g = np.asarray(br.gradient_cd(P, x), dtype=np.float64) / 2
    c_end = float(br.true_cost(P, x.astype(LD)))
    m = float(g @ np.linalg.solve(H, g))
    print(f"radial {radial}: g'H^-1 g {m:.2e}, cost {c_end:.4g}, error_ {err}")
    assert len(err) >= 2 and m <= 1e-9 * c_end


def test_undistortion_inverts_the_distortion():
    """r (1 + k1 r^2 + k2 r^4) of the mpmath undistortion's r is rd to 1e-15
    relative over r in [0, 0.7] at K_TRUE (the distortion as radial_ref writes
    it: d = (1 + k1 r2) + (k2 r2) r2), and a measurement past the fold of a
    strong lens fails."""
    import mpmath as mp
    k1, k2 = rad.K_TRUE
    worst = 0.0
    with mp.workdps(40):
        for r in np.linspace(0.0, 0.7, 71):
            r = mp.mpf(float(r))
            r2 = r * r
            rd = r * ((1 + k1 * r2) + (k2 * r2) * r2)
            got = br.undistort_r_mp(k1, k2, float(rd))
            assert got is not None
            back = got * ((1 + k1 * got * got) + (k2 * got * got) * got * got)
            if rd != 0:
                worst = max(worst, float(abs(back - mp.mpf(float(rd))) / mp.mpf(float(rd))))
                assert abs(got - r) <= 1e-15 * r
    print(f"undistortion: worst relative error {worst:.2e}")
    assert worst <= 1e-15
    # k1 = -0.5: r d(r) peaks at r^2 = 2/3 with rd = 0.5443...; 0.6 is past the fold
    assert br.undistort_r_mp(-0.5, 0.0, 0.6) is None
    assert br.undistort_r_mp(-0.5, 0.0, 0.5) is not None
    # the pixel form: f n + c with n = nd r / rd
    u = br.undistort_mp(800.0, (500.0, 400.0), k1, k2, (700.0, 300.0))
    n = (u - np.array([500.0, 400.0])) / 800.0
    r2 = float(n @ n)
    back = 800.0 * ((1 + k1 * r2) + (k2 * r2) * r2) * n + np.array([500.0, 400.0])
    assert np.allclose(back, [700.0, 300.0], rtol=0, atol=1e-10)


# ---------------------------------------------------------------------------
# header, binding, argument checks (no device work)
# ---------------------------------------------------------------------------
NEW = ("vlgba_resect_ex", "vlgba_intersect_ex", "vlgba_triangulate_ex")
E_ARG, E_NUMA = -1001, -1002


def test_header_and_binding_declare_the_new_entries():
    from bundleadjustmentmatlab_amd import _lib
    import bundleadjustmentmatlab_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "vlgba.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(vlgba_\w+)\s*\(", src))
    for nm in NEW:
        assert nm in names and nm in _lib.SIGNATURES
        assert hasattr(pkg.lib(), nm)
        # the binding's argument count is the header's
        decl = re.search(r"\b" + nm + r"\s*\(([^;]*)\)\s*;", src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[nm][1]), nm
    assert "#define VLGBA_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6
    import inspect
    for fn, kws in ((pkg.bundle_euclid_resect, ("radial", "jacobian", "loss", "loss_scale",
                                                 "return_residuals")),
                    (pkg.bundle_euclid_intersect, ("radial", "jacobian", "loss", "loss_scale",
                                                    "return_residuals")),
                    (pkg.triangulate_points, ("radial",))):
        assert set(kws) <= set(inspect.signature(fn).parameters)


def _resect_ex(na=6, nprob=1, jac=0, loss=0, scale=0.0, ptr=(0, 2), null=(), cap=0):
    import bundleadjustmentmatlab_amd as pkg
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, VlgbaResectProblem, c_dp
    llp = ctypes.POINTER(ctypes.c_longlong)
    ptr = np.asarray(ptr, dtype=np.int64)
    N = int(max(ptr.max(), 1))
    X, x, K, a = np.ones(3 * N), np.zeros(2 * N), np.ones(4 * max(nprob, 1)), np.zeros(12)
    p = lambda nm, v: None if nm in null else v.ctypes.data_as(c_dp)
    pr = VlgbaResectProblem(nprob, na, None if "ptr" in null else ptr.ctypes.data_as(llp),
                            p("X", X), p("x", x), p("K", K))
    opt = VlgbaOptions()
    return pkg.lib().vlgba_resect_ex(None if "prob" in null else ctypes.byref(pr),
                                     ctypes.byref(opt), jac, loss, scale, p("a", a), None, cap,
                                     None, None, None, None)


def test_resect_ex_arguments_rejected_before_device_work():
    for nm in ("prob", "a", "ptr", "X", "x", "K"):
        assert _resect_ex(null=(nm,)) == E_ARG, nm
    for na in (5, 8, 11, 12):
        assert _resect_ex(na=na) == E_NUMA, na
    assert _resect_ex(na=9, jac=0) == E_ARG                 # the radial model is analytic only
    assert _resect_ex(jac=2) == E_ARG and _resect_ex(jac=-1) == E_ARG
    assert _resect_ex(loss=3) == E_ARG and _resect_ex(loss=-1) == E_ARG
    for sc in (0.0, -1.0, float("inf"), float("nan")):
        assert _resect_ex(loss=1, scale=sc) == E_ARG and _resect_ex(loss=2, scale=sc) == E_ARG
    assert _resect_ex(ptr=(1, 2)) == E_ARG and _resect_ex(ptr=(0, -1)) == E_ARG
    assert _resect_ex(nprob=-1) == E_ARG
    # nprob == 0 succeeds without a launch, in every valid mode
    assert _resect_ex(nprob=0, ptr=(0,)) == 0
    assert _resect_ex(na=9, nprob=0, jac=1, loss=2, scale=3.0, ptr=(0,)) == 0
    assert _resect_ex(na=9, nprob=0, jac=0, ptr=(0,)) == E_ARG
    # the plain entry still refuses the radial model
    import bundleadjustmentmatlab_amd as pkg
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, VlgbaResectProblem, c_dp
    ptr = np.zeros(1, dtype=np.int64)
    a = np.zeros(9)
    pr = VlgbaResectProblem(0, 9, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), None,
                            None, None)
    assert pkg.lib().vlgba_resect(ctypes.byref(pr), ctypes.byref(VlgbaOptions()),
                                  a.ctypes.data_as(c_dp), None, 0, None, None) == E_NUMA


def _args(m=2, n=2, ptr=(0, 2, 4), cam=(0, 1, 1, 0)):
    return dict(m=m, K=np.tile([500.0, 500.0, 250.0, 250.0], m), T=np.zeros(3 * m),
                w=np.zeros(3 * m), kd=np.zeros(2 * m), n=n, ptr=np.asarray(ptr, dtype=np.int64),
                cam=np.asarray(cam, dtype=np.int32), x=np.zeros(2 * len(cam)))


def _call(which, a, null=("kd",), jac=0, loss=0, scale=0.0):
    import bundleadjustmentmatlab_amd as pkg
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, c_dp, c_ip
    L = pkg.lib()
    llp = ctypes.POINTER(ctypes.c_longlong)
    p = {k: (None if k in null else
             a[k].ctypes.data_as(llp if k == "ptr" else c_ip if k == "cam" else c_dp))
         for k in ("K", "T", "w", "kd", "ptr", "cam", "x")}
    Xb = np.zeros(4 * max(a["n"], 1))
    Xp = None if "X" in null else Xb.ctypes.data_as(c_dp)
    if which == "triangulate":
        return L.vlgba_triangulate_ex(a["m"], p["K"], p["T"], p["w"], p["kd"], a["n"], p["ptr"],
                                      p["cam"], p["x"], 0, Xp, None)
    opt = VlgbaOptions()
    return L.vlgba_intersect_ex(a["m"], p["K"], p["T"], p["w"], p["kd"], a["n"], p["ptr"],
                                p["cam"], p["x"], ctypes.byref(opt), jac, loss, scale, Xp, None, 0,
                                None, None, None, None)


@pytest.mark.parametrize("which", ["triangulate", "intersect"])
@pytest.mark.parametrize("radial", [False, True])
def test_per_point_ex_arguments_rejected_before_device_work(which, radial):
    base = () if radial else ("kd",)
    kw = dict(jac=1) if radial else {}
    for nm in ("K", "T", "w", "ptr", "cam", "x", "X"):
        assert _call(which, _args(), null=base + (nm,), **kw) == E_ARG, nm
    assert _call(which, dict(_args(), m=0), null=base, **kw) == E_ARG
    assert _call(which, dict(_args(), n=-1), null=base, **kw) == E_ARG
    assert _call(which, _args(ptr=(0, 3, 2)), null=base, **kw) == E_ARG
    assert _call(which, _args(ptr=(1, 2, 4)), null=base, **kw) == E_ARG
    assert _call(which, _args(cam=(0, 1, 2, 0)), null=base, **kw) == E_ARG
    assert _call(which, _args(cam=(0, -1, 1, 0)), null=base, **kw) == E_ARG
    assert _call(which, _args(n=0, ptr=(0,), cam=()), null=base, **kw) == 0
    assert _call(which, _args(n=0, ptr=(0,), cam=()), null=base + ("cam", "x"), **kw) == 0


def test_intersect_ex_mode_arguments():
    a = _args(n=0, ptr=(0,), cam=())
    assert _call("intersect", a, null=(), jac=0) == E_ARG          # radial is analytic only
    assert _call("intersect", a, null=(), jac=1) == 0
    assert _call("intersect", a, jac=2) == E_ARG
    assert _call("intersect", a, loss=3) == E_ARG
    for sc in (0.0, -2.0, float("nan"), float("inf")):
        assert _call("intersect", a, loss=1, scale=sc) == E_ARG
    assert _call("intersect", a, loss=2, scale=1.5) == 0
    assert _call("intersect", a, loss=0, scale=-1.0) == 0           # the scale is unused


def test_python_mirrors():
    """the keyword checks of the Python layer, and the empty batches"""
    import bundleadjustmentmatlab_amd as pkg
    K = np.tile([[500.0], [500.0], [250.0], [250.0]], (1, 2))
    z = np.zeros((3, 2))
    kd = np.zeros((2, 2))
    X = pkg.triangulate_points(K, z, z, [0], [], np.zeros((0, 2)), radial=kd)
    assert X.shape == (4, 0)
    out = pkg.bundle_euclid_intersect(K, z, z, np.zeros((3, 0)), [0], [], np.zeros((0, 2)),
                                      radial=kd, loss="huber", loss_scale=2.0,
                                      return_residuals=True)
    assert out[0].shape == (3, 0) and out[1] == [] and out[2][0].shape == (0, 2)
    with pytest.raises(pkg.VlgbaError):       # radial with forward differences
        pkg.bundle_euclid_intersect(K, z, z, np.zeros((3, 0)), [0], [], np.zeros((0, 2)),
                                    radial=kd, jacobian="fd")
    with pytest.raises(ValueError):
        pkg.bundle_euclid_intersect(K, z, z, np.zeros((3, 0)), [0], [], np.zeros((0, 2)),
                                    loss="tukey")
    with pytest.raises(ValueError):
        pkg.bundle_euclid_resect(K, z, z, [], [], jacobian="auto")
    with pytest.raises(ValueError):
        pkg.triangulate_points(K, z, z, [0], [], np.zeros((0, 2)), radial=np.zeros((2, 3)))
