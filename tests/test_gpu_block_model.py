"""GPU: the batched one-camera / one-point entries with a camera model, a
Jacobian mode and a loss (vlgba_resect_ex, vlgba_intersect_ex,
vlgba_triangulate_ex) against the one-block references of tests/block_ref.py.

Shapes: cameras of 0, 6, 255, 256, 257 and 513 observations (RS_TILE is 256)
alone and in a batch of 72; points in batches of 1, 63, 64, 65 and 130 (64-lane
workgroups) with tracks of 0, 1, 2, 3 and 9 views.  Radial scenes: the lens
radial_ref.K_TRUE, 0.5 px noise, the start's coefficients 10 % / 20 % off.

Bars.
  bit identities       np.array_equal.
  cost, residuals, w   within the references' own propagated bounds (ratio <= 1):
                       block_ref.cost / residuals / weights restate the kernels'
                       evaluation with every fp64 rounding bounded; error_ =
                       cost / views adds one rounding.
  CPU cost at the end  1e-12 relative to error_(end) (tests/test_gpu_intersect.py).
  one pass             the backward error of the step d = x_new - x in the
                       reference's long double damped system Hs d = g at the
                       pass's lambda, entry by entry:
                         |Hs d - g|_i <= sum_j dHs_ij |d_j| + dg_i + solve_i
                                          + sum_j |Hs_ij| u |x_new_j|
                       dHs, dg: the linearisation's propagated bounds (the diagonal
                       times (1 + lambda), plus two roundings for that product);
                       the last term: d is recovered from the rounded x_new = x +
                       d.  solve, camera block: sum_j (3 n + 2) u sqrt(Hs_ii Hs_jj)
                       |d_j|, the sequential Cholesky solve's backward error |dH|
                       <= gamma_{3n+1} |L||L'| with |L||L'|_ij <= sqrt(h_ii h_jj)
                       (Higham, Accuracy and Stability, Thm 10.4).  solve, 3 x 3
                       point block: the step is d = (adj(Hs) / det) g evaluated in
                       closed form (vlg_pinv3), so solve = |Hs| dd with dd the
                       first-order forward bound of that evaluation, operation by
                       operation: a cofactor a b - c d carries 2 u (|a b| + |c d|)
                       =: 2 u C^; det = sum_j m_0j c_0j carries ddet = 5 u sum_j
                       |m_0j| C^_0j (the cofactors' 2 u and 3 u for each product and
                       the sum's additions); V^-1 = c (1 / det) adds two
                       roundings: dV = (2 u C^ + |c| (ddet / |det| + 2 u)) / |det|;
                       d = V^-1 g three more: dd = dV |g| + 3 u |V^-1| |g|.  No
                       entrywise comparison of the step: the radial 9 x 9 block
                       is ill-conditioned.
  converged            block_ref.block_lm started at the GPU's answer lowers the
                       cost by at most 1e-6 relative (the project's restart bar).
  triangulation        against triang_ref.triangulate_mp on observations
                       undistorted in mpmath (block_ref.undistort_mp): the GPU's
                       error at most 16 x numpy's SVD's on the same rows, the bar
                       of tests/test_gpu_triangulate.py.
"""
import functools

import numpy as np
import pytest

import block_ref as br
import radial_ref as rad
import robust_ref as rr
import triang_ref as tr

pytestmark = pytest.mark.gpu

LD = br.LD
U53 = float(br.U53)
STOP = rad.E2E["stop"]
OPTS = {6: ("fix_calibration",), 7: ("fix_principal",), 10: (), 9: ()}
SIZES = (0, 6, 255, 256, 257, 513)
HUGE = 1e150


# ---------------------------------------------------------------------------
# helpers: batches of block_ref problems through the Python layer
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cam(N, seed, na, w0_zero=False):
    return br.synth_camera(N, seed, na, w0_zero=w0_zero)


def _resect(gpu, probs, na, **kw):
    """the batch through bundle_euclid_resect -> list of dict(a, err, e, w) per
    camera (a: the returned parameter vector), and the stats"""
    c = len(probs)
    a0 = np.stack([P["a"][:, 0] for P in probs], 1) if c else np.zeros((na, 0))
    K = np.stack([P["K"][:, 0] for P in probs], 1) if c else np.zeros((4, 0))
    K = K.copy()
    if na in (7, 9):
        K[0] = a0[6]
    elif na == 10:
        K[:] = a0[6:10]
    if na == 9:
        kw = dict(kw, radial=a0[7:9])
    out = gpu.bundle_euclid_resect(K, a0[3:6], a0[0:3], [P["b"] for P in probs],
                                   [P["obs_x"].T for P in probs], *OPTS[na], return_stats=True,
                                   return_residuals=True, **kw)
    K_, T_, w_, errs, st, res = out[:6]
    a = np.zeros((na, c))
    a[0:3], a[3:6] = w_, T_
    if na == 7:
        a[6] = K_[0]
    elif na == 10:
        a[6:10] = K_
    elif na == 9:
        a[6], a[7:9] = K_[0], out[6]
    return [dict(a=a[:, q], err=errs[q], e=res[q][0].T, w=res[q][1]) for q in range(c)], st


def _same(r, s):
    return (np.array_equal(r["a"], s["a"]) and np.array_equal(r["err"], s["err"]) and
            np.array_equal(r["e"], s["e"]) and np.array_equal(r["w"], s["w"]))


def _isect(gpu, s, X0=None, sel=None, **kw):
    """points ``sel`` (default all) of a synth_tracks batch through
    bundle_euclid_intersect -> (X (3, n), errs, (e, w), stats)"""
    sel = np.arange(s["n"]) if sel is None else np.asarray(sel)
    cl = [s["cam"][s["ptr"][i]:s["ptr"][i + 1]] for i in sel]
    xl = [s["x"][s["ptr"][i]:s["ptr"][i + 1]] for i in sel]
    X0 = s["X0"] if X0 is None else X0
    if s["kd"] is not None:
        kw = dict(kw, radial=s["kd"])
    X, errs, st, res = gpu.bundle_euclid_intersect(s["K"], s["T"], s["w"], X0[:, sel],
                                                   *tr.pack(cl, xl), return_stats=True,
                                                   return_residuals=True, **kw)
    return X, errs, res, st


VIEWS = (0, 1, 2, 3, 9)


@functools.lru_cache(maxsize=None)
def _tracks(n, radial, seed=7):
    return br.synth_tracks([VIEWS[i % len(VIEWS)] for i in range(n)], seed + n, radial)


def _ratio(got, ref, bound):
    return rr.ratio(got, ref, bound)


# ---------------------------------------------------------------------------
# 1. nothing moved
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("num_a", [6, 7, 10])
def test_resect_ex_defaults_equal_vlgba_resect(gpu, num_a):
    import test_gpu_resect as old
    K, T, w, Xs, xs = old._cameras(num_a=num_a)
    opts = old.OPTS[num_a]
    ref = gpu.bundle_euclid_resect(K, T, w, Xs, xs, *opts)
    got = gpu.bundle_euclid_resect(K, T, w, Xs, xs, *opts, return_residuals=True)
    assert all(np.array_equal(g, r) for g, r in zip(got[:3], ref[:3]))
    assert all(np.array_equal(g, r) for g, r in zip(got[3], ref[3]))
    assert all(np.all(wq == 1.0) and e.shape == (2, X.shape[1])
               for (e, wq), X in zip(got[4], Xs))


def test_resect_ex_defaults_equal_vlgba_resect_on_the_large_batch(gpu):
    """the batch of test_resect_batch_large: every camera of config 3"""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg3")
    order = np.argsort(sc.obs_cam, kind="stable")
    cam, pt = sc.obs_cam[order], sc.obs_pt[order]
    # (the C entries on flat arrays: the Python layer's per-camera lists would
    # take most of this test's time)
    import ctypes
    from bundleadjustmentmatlab_amd._lib import (VlgbaOptions, VlgbaResectProblem, VlgbaStats,
                                                 c_dp, c_ip)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=sc.m))]).astype(np.int64)
    X = np.ascontiguousarray(sc.X[:3, pt].T)
    x = np.ascontiguousarray(sc.obs_x[order])
    K = np.ascontiguousarray(sc.K.T)
    a0 = np.ascontiguousarray(np.vstack([sc.w0, sc.T0]).T)
    dp = lambda q: q.ctypes.data_as(c_dp)
    pr = VlgbaResectProblem(sc.m, 6, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                            dp(X), dp(x), dp(K))
    opt, cap = VlgbaOptions(), 21
    out = []
    for ex in (False, True):
        a, err, nerr, st = a0.copy(), np.zeros((sc.m, cap)), np.zeros(sc.m, np.int32), VlgbaStats()
        tail = (dp(a), dp(err), cap, nerr.ctypes.data_as(c_ip))
        if ex:
            rc = gpu.lib().vlgba_resect_ex(ctypes.byref(pr), ctypes.byref(opt), 0, 0, 0.0, *tail,
                                           None, None, ctypes.byref(st))
        else:
            rc = gpu.lib().vlgba_resect(ctypes.byref(pr), ctypes.byref(opt), *tail,
                                        ctypes.byref(st))
        assert rc == 0
        out.append((a, err, nerr))
    assert all(np.array_equal(p, q) for p, q in zip(*out))
    assert np.all(out[0][2] >= 2) and not np.array_equal(out[0][0], a0)


@pytest.mark.parametrize("which", ["short", "long"])
def test_intersect_ex_defaults_equal_vlgba_intersect(gpu, which):
    import test_gpu_intersect as old
    sc, cl, xl, X0 = old._batch_short() if which == "short" else old._batch_long()
    csr = tr.pack(cl, xl)
    X_, errs = gpu.bundle_euclid_intersect(sc.K, sc.T, sc.w, X0, *csr)
    Xe, errs_e, (e, wt) = gpu.bundle_euclid_intersect(sc.K, sc.T, sc.w, X0, *csr,
                                                      return_residuals=True)
    assert np.array_equal(X_, Xe) and len(errs) == len(errs_e)
    assert all(np.array_equal(p, q) for p, q in zip(errs, errs_e))
    assert np.all(wt == 1.0) and e.shape == (len(csr[1]), 2)


def test_intersect_ex_defaults_equal_vlgba_intersect_on_20000_points(gpu):
    """the batch of test_batch_of_20000_points"""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=50, n=20_000, track=6, seed=9)
    ptr = np.searchsorted(sc.obs_pt, np.arange(sc.n + 1)).astype(np.int64)
    X0 = sc.X.copy()
    X0[:3] += 0.05
    args = (sc.K, sc.T, sc.w, X0, ptr, sc.obs_cam, sc.obs_x)
    X_, errs = gpu.bundle_euclid_intersect(*args)
    Xe, errs_e, (e, wt) = gpu.bundle_euclid_intersect(*args, return_residuals=True)
    assert np.array_equal(X_, Xe) and len(errs_e) == sc.n
    assert all(np.array_equal(p, q) for p, q in zip(errs, errs_e))
    assert np.all(wt == 1.0)


def test_triangulate_ex_without_a_lens_equals_vlgba_triangulate(gpu):
    import ctypes
    from bundleadjustmentmatlab_amd._lib import c_dp, c_ip
    from bundleadjustmentmatlab_amd.bundle import _tracks as csr_args
    import test_gpu_triangulate as old
    sc = old._scene(m=6, min_n=260, max_n=300, seed=4)
    ptr, cam, x = tr.tracks(sc)
    X, st = gpu.triangulate_points(sc.K, sc.T, sc.w, ptr, cam, x, return_status=True)
    keep, args = csr_args(sc.K, sc.T, sc.w, ptr, cam, x)
    Xe, ste = np.zeros((4, args[4]), order="F"), np.zeros(args[4], dtype=np.int32)
    rc = gpu.lib().vlgba_triangulate_ex(*args[:4], None, *args[4:], 0, Xe.ctypes.data_as(c_dp),
                                        ste.ctypes.data_as(c_ip))
    assert rc == 0 and np.array_equal(Xe, X) and np.array_equal(ste, st)
    assert set(np.unique(st)) >= {1}


# ---------------------------------------------------------------------------
# 2. mode identities, bit for bit
# ---------------------------------------------------------------------------
MODES = [(6, "fd"), (6, "analytic"), (7, "fd"), (7, "analytic"), (10, "fd"), (10, "analytic"),
         (9, "analytic")]


@pytest.mark.parametrize("na,jac", MODES)
def test_resect_identities(gpu, na, jac):
    """Huber at 1e150 = no loss; alone = in the batch = in a permuted batch; two
    calls the same bits; every size of SIZES, in a batch of 72."""
    probs = [_cam(SIZES[q % len(SIZES)], 100 + q, na)[0] for q in range(72)]
    base, st = _resect(gpu, probs, na, jacobian=jac)
    again, _ = _resect(gpu, probs, na, jacobian=jac)
    hub, _ = _resect(gpu, probs, na, jacobian=jac, loss="huber", loss_scale=HUGE)
    perm = np.random.default_rng(1).permutation(len(probs))
    shuf, _ = _resect(gpu, [probs[q] for q in perm], na, jacobian=jac)
    for q in range(len(probs)):
        assert _same(base[q], again[q]) and _same(base[q], hub[q]), q
        assert _same(base[perm[q]], shuf[q]), q
    for q in range(len(SIZES)):
        alone, _ = _resect(gpu, [probs[q]], na, jacobian=jac)
        assert _same(alone[0], base[q]), SIZES[q]
        assert len(base[q]["err"]) >= 2 or SIZES[q] == 0
    print(f"na {na} {jac}: passes {st.iterations}, accepted {st.accepted}; error_ of the 513: "
          f"{base[5]['err']}")
    assert len(base[0]["err"]) == 0 and np.array_equal(base[0]["a"], probs[0]["a"][:, 0])


@pytest.mark.parametrize("na", [6, 7, 10])
def test_analytic_start_cost_is_the_fd_start_cost(gpu, na):
    probs = [_cam(N, 100 + q, na)[0] for q, N in enumerate(SIZES)]
    fd, _ = _resect(gpu, probs, na, jacobian="fd")
    an, _ = _resect(gpu, probs, na, jacobian="analytic")
    for q in range(1, len(SIZES)):
        assert fd[q]["err"][0] == an[q]["err"][0], SIZES[q]
    for loss in ("huber", "cauchy"):
        f2, _ = _resect(gpu, probs, na, jacobian="fd", loss=loss, loss_scale=1.0)
        a2, _ = _resect(gpu, probs, na, jacobian="analytic", loss=loss, loss_scale=1.0)
        for q in range(1, len(SIZES)):
            assert f2[q]["err"][0] == a2[q]["err"][0] < fd[q]["err"][0], (loss, SIZES[q])


@pytest.mark.parametrize("radial,jac", [(False, "fd"), (False, "analytic"), (True, "analytic")])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_intersect_identities(gpu, n, radial, jac):
    s = _tracks(n, radial)
    X, errs, (e, wt), st = _isect(gpu, s, jacobian=jac)
    X2, errs2, (e2, w2), _ = _isect(gpu, s, jacobian=jac)
    Xh, errsh, (eh, wh), _ = _isect(gpu, s, jacobian=jac, loss="huber", loss_scale=HUGE)
    for got in ((X2, errs2, e2, w2), (Xh, errsh, eh, wh)):
        assert np.array_equal(got[0], X) and np.array_equal(got[2], e)
        assert np.array_equal(got[3], wt)
        assert all(np.array_equal(p, q) for p, q in zip(got[1], errs))
    perm = np.random.default_rng(2).permutation(n)
    Xp, errsp, _, _ = _isect(gpu, s, sel=perm, jacobian=jac)
    for k, i in enumerate(perm):
        assert np.array_equal(Xp[:, k], X[:, i]) and np.array_equal(errsp[k], errs[i])
    for i in range(min(n, len(VIEWS))):
        Xa, ea, _, _ = _isect(gpu, s, sel=[i], jacobian=jac)
        assert np.array_equal(Xa[:, 0], X[:, i]) and np.array_equal(ea[0], errs[i])
        if VIEWS[i] == 0:       # a point without views is left untouched
            assert len(errs[i]) == 0 and np.array_equal(X[:, i], s["X0"][:, i])
        elif VIEWS[i] >= 2:
            assert len(errs[i]) >= 2
    if not radial and jac == "analytic":
        Xf, errsf, _, _ = _isect(gpu, s, jacobian="fd")
        assert all(len(p) == 0 or p[0] == q[0] for p, q in zip(errs, errsf))


# ---------------------------------------------------------------------------
# 3. cost, residuals and weights against the references
# ---------------------------------------------------------------------------
def _check_outputs(P, r, kind, c, tag):
    """error_[0] at the start, error_[-1], res_out and w_out at the returned
    parameters within the references' bounds; the CPU cost at the end 1e-12"""
    N = len(P["pt"])
    c0, c0b = br.cost(P, kind=kind, c=c)
    a, b = br.with_free(P, r["x"])
    c1, c1b = br.cost(P, a, b, kind, c)
    r0 = _ratio(r["err"][0], c0 / N, (c0b + float(U53) * c0) / N)
    r1 = _ratio(r["err"][-1], c1 / N, (c1b + float(U53) * c1) / N)
    e, eb = br.residuals(P, a, b)
    re = _ratio(r["e"], e, eb)
    w, wb = br.weights(P, a, b, kind, c)
    rw = _ratio(r["w"], w, wb)
    # the CPU cost of the 1e-12 bar: plain fp64 in the kernels' own operation
    # order (block_ref.cost_fp64), so that a near-zero residual -- a two-view
    # point can end at 1e-2 px -- is not charged with the reference's rounding
    rel = abs(br.cost_fp64(P, a, b, kind, c) / N - r["err"][-1]) / r["err"][-1]
    print(f"{tag}: ratios start {r0:.3f} end {r1:.3f} residuals {re:.3f} weights {rw:.3f}; "
          f"CPU cost at the end vs error_(end) {rel:.1e}")
    assert max(r0, r1, re, rw) <= 1.0
    assert rel <= 1e-12
    return w


CASES3 = [(6, "fd", "none"), (7, "analytic", "none"), (10, "analytic", "cauchy"),
          (9, "analytic", "none"), (9, "analytic", "huber"), (6, "analytic", "huber")]


@pytest.mark.parametrize("na,jac,kind", CASES3)
def test_resect_outputs_within_the_reference_bounds(gpu, na, jac, kind):
    for N in (6, 257, 513):
        P = dict(_cam(N, 300 + N, na)[0])
        if kind != "none":
            P["obs_x"], _ = rr.plant_outliers(P["obs_x"], frac=0.1, seed=N)
        (r,), _ = _resect(gpu, [P], na, jacobian=jac, loss=kind, loss_scale=2.0)
        r["x"] = r["a"]
        w = _check_outputs(P, r, kind, 2.0, f"resect na {na} {jac} {kind} N {N}")
        assert kind == "none" or np.all(r["w"] <= 1.0)
        assert kind == "none" or N < 257 or w.min() < 1


@pytest.mark.parametrize("radial,jac,kind", [(False, "fd", "none"), (False, "analytic", "cauchy"),
                                             (True, "analytic", "none"), (True, "analytic", "huber")])
def test_intersect_outputs_within_the_reference_bounds(gpu, radial, jac, kind):
    s = dict(_tracks(65, radial))
    if kind != "none":
        s["x"], _ = rr.plant_outliers(s["x"], frac=0.1, seed=5)
    X, errs, (e, wt), _ = _isect(gpu, s, jacobian=jac, loss=kind, loss_scale=2.0)
    for i in range(s["n"]):         # every point of both workgroups with two views or more
        sl = slice(s["ptr"][i], s["ptr"][i + 1])
        if sl.stop - sl.start < 2:
            continue
        P = br.track_point(s, i)
        _check_outputs(P, dict(x=X[:, i], err=errs[i], e=e[sl], w=wt[sl]), kind, 2.0,
                       f"intersect radial {radial} {jac} {kind} point {i} ({sl.stop - sl.start} views)")


# ---------------------------------------------------------------------------
# 4. one pass: the backward error of the first accepted step
# ---------------------------------------------------------------------------
def _adjugate_forward(Hs, g):
    """dd of the module docstring: the first-order rounding bound of
    d = (adj(Hs) / det(Hs)) g as vlg_pinv3 evaluates it (long double)"""
    M, u = np.asarray(Hs, dtype=LD), br.U53
    C, Ca = np.zeros((3, 3), dtype=LD), np.zeros((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            (r0, r1), (c0, c1) = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            p, q = M[r0, c0] * M[r1, c1], M[r0, c1] * M[r1, c0]
            C[i, j], Ca[i, j] = (-1) ** (i + j) * (p - q), abs(p) + abs(q)
    det = (M[0] * C[0]).sum()
    ddet = 5 * u * (np.abs(M[0]) * Ca[0]).sum()
    dV = (2 * u * Ca.T + np.abs(C.T) * (ddet / abs(det) + 2 * u)) / abs(det)
    ag = np.abs(np.asarray(g, dtype=LD))
    return dV @ ag + 3 * u * (np.abs(C.T) / abs(det)) @ ag


def _backward_ratio(P, x_new, passes, kind, c):
    """largest |Hs d - g|_i / bound_i of the step d = x_new - x at the lambda of
    the run's last pass (the passes before it were rejected: lambda0 2^(k(k+1)/2))"""
    k = passes - 1
    lam = 1e-3 * 2.0 ** (k * (k + 1) // 2)
    H, g, Hb, gb = br.block(P, br.linearization(P, kind=kind, c=c))
    n = len(g)
    Hs = br.damped(H, LD(lam))
    Hsb = br.damped(Hb, LD(lam))
    dd = np.sqrt(np.diag(Hs))
    Hsb[np.arange(n), np.arange(n)] += 2 * br.U53 * np.diag(Hs)
    x = br.free(P).astype(LD)
    d = np.asarray(x_new, dtype=np.float64).astype(LD) - x
    r = np.abs(Hs @ d - g)
    if n == 3:
        solve = np.abs(Hs) @ _adjugate_forward(Hs, g)
    else:
        solve = ((3 * n + 2) * br.U53 * np.outer(dd, dd)) @ np.abs(d)
    bound = (Hsb @ np.abs(d) + gb + solve +
             np.abs(Hs) @ (br.U53 * np.abs(np.asarray(x_new, dtype=LD))))
    scale = np.abs(Hs) @ np.abs(d)
    return float((r / bound).max()), float((r / scale).max()), lam


@pytest.mark.parametrize("na,jac,kind", [(6, "analytic", "none"), (7, "analytic", "none"),
                                         (10, "analytic", "none"), (9, "analytic", "none"),
                                         (9, "analytic", "huber"), (10, "analytic", "cauchy")])
def test_resect_one_pass_backward_error(gpu, na, jac, kind):
    for N in (257, 513):
        P = dict(_cam(N, 400 + N, na)[0])
        if kind != "none":
            P["obs_x"], _ = rr.plant_outliers(P["obs_x"], frac=0.05, seed=N)
        (r,), st = _resect(gpu, [P], na, jacobian=jac, loss=kind, loss_scale=2.0, max_iter=2)
        assert len(r["err"]) == 2 and st.accepted == 1
        ratio, rel, lam = _backward_ratio(P, r["a"], st.iterations, kind, 2.0)
        print(f"one pass resect na {na} {kind} N {N}: lambda {lam:g}, backward error / bound "
              f"{ratio:.3f}, relative to |Hs||d| {rel:.1e}")
        assert ratio <= 1.0


@pytest.mark.parametrize("radial,kind", [(False, "none"), (True, "none"), (True, "cauchy")])
def test_intersect_one_pass_backward_error(gpu, radial, kind):
    s = _tracks(5, radial)
    for i in (2, 3, 4):
        X, errs, _, st = _isect(gpu, s, sel=[i], jacobian="analytic", loss=kind, loss_scale=2.0,
                                max_iter=2)
        assert len(errs[0]) == 2 and st.accepted == 1
        ratio, rel, lam = _backward_ratio(br.track_point(s, i), X[:, 0], st.iterations, kind, 2.0)
        print(f"one pass intersect radial {radial} {kind} {VIEWS[i]} views: lambda {lam:g}, "
              f"backward error / bound {ratio:.3f}, relative {rel:.1e}")
        assert ratio <= 1.0


# ---------------------------------------------------------------------------
# 5. converged: the reference LM from the GPU's answer
# ---------------------------------------------------------------------------
def _restart_drop(P, x, kind, c):
    a, b = br.with_free(P, x)
    at = float(br.cost(P, a, b, kind, c)[0])
    Q = dict(P, a=a, b=b)
    _, err = br.block_lm(Q, kind, c, **STOP)
    final = err[-1] * len(P["pt"]) if len(err) else at
    return (at - final) / at, at


CASES5 = [(9, "none"), (6, "none"), (7, "none"), (10, "none"), (9, "huber"), (9, "cauchy"),
          (6, "huber"), (6, "cauchy")]


@pytest.mark.parametrize("na,kind", CASES5)
def test_resect_converged_survives_the_reference_restart(gpu, na, kind):
    P = dict(_cam(257, 500 + na, na)[0])
    if kind != "none":
        P["obs_x"], out = rr.plant_outliers(P["obs_x"], seed=na)
        assert out.sum() >= 3
    (r,), st = _resect(gpu, [P], na, jacobian="analytic", loss=kind, loss_scale=3.0, **STOP)
    drop, at = _restart_drop(P, r["a"], kind, 3.0)
    print(f"converged resect na {na} {kind}: error_ {r['err'][0]:.6g} -> {r['err'][-1]:.12g} in "
          f"{st.iterations} passes; the reference LM from there drops {drop:.2e}")
    assert r["err"][-1] < r["err"][0] and -1e-12 <= drop <= 1e-6


def test_radial_huber_camera_agrees_with_the_fused_solver(gpu):
    """second witness: BundleAdjuster(num_a=9, fix_structure=True) on the same
    one-camera problem ends at the same robust cost to 1e-6"""
    P = dict(_cam(257, 509, 9)[0])
    P["obs_x"], _ = rr.plant_outliers(P["obs_x"], seed=9)
    (r,), _ = _resect(gpu, [P], 9, loss="huber", loss_scale=3.0, **STOP)
    with gpu.BundleAdjuster(P["K"], P["pt"], P["cam"], P["obs_x"], P["n"], 9, fix_structure=True,
                            loss="huber", loss_scale=3.0, **STOP) as ba:
        ba.set_params(P["a"], P["b"])
        err, _ = ba.run()
        a1, _ = ba.get_params()
    c_ba = float(br.cost(P, a1, P["b"], "huber", 3.0)[0])
    c_rs = float(br.cost(P, *br.with_free(P, r["a"]), "huber", 3.0)[0])
    print(f"fused solver cost {c_ba:.12g} ({len(err)} error_ entries), resect_ex {c_rs:.12g}, "
          f"relative difference {abs(c_ba - c_rs) / c_ba:.2e}")
    assert abs(c_ba - c_rs) <= 1e-6 * c_ba


@pytest.mark.parametrize("radial,kind", [(True, "none"), (False, "none"), (True, "huber"),
                                         (False, "cauchy")])
def test_intersect_converged_survives_the_reference_restart(gpu, radial, kind):
    s = dict(_tracks(65, radial))
    if kind != "none":
        s["x"], _ = rr.plant_outliers(s["x"], frac=0.05, seed=3)
    X, errs, _, _ = _isect(gpu, s, jacobian="analytic", loss=kind, loss_scale=3.0, **STOP)
    worst = -1.0
    for i in range(15):
        if VIEWS[i % len(VIEWS)] < 2:
            continue
        drop, at = _restart_drop(br.track_point(s, i), X[:, i], kind, 3.0)
        worst = max(worst, drop)
        assert -1e-12 <= drop <= 1e-6, (i, drop)
    print(f"converged intersect radial {radial} {kind}: worst restart drop {worst:.2e}")


# ---------------------------------------------------------------------------
# 6. the reason for the analytic mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("na", [6, 7, 10])
def test_a_camera_started_at_zero_rotation(gpu, na):
    P, a_true = _cam(257, 600 + na, na, w0_zero=True)
    assert np.all(P["a"][0:3] == 0) and np.linalg.norm(a_true[0:3]) > 0.019
    (fd,), _ = _resect(gpu, [P], na, jacobian="fd")
    (an,), _ = _resect(gpu, [P], na, jacobian="analytic")
    print(f"w = 0 start, na {na}: FD ends at w {fd['a'][0:3]} error_ {fd['err'][-1]:.4g}; "
          f"analytic at w {an['a'][0:3]} error_ {an['err'][-1]:.4g}; truth {a_true[0:3]}")
    assert np.all(fd["a"][0:3] == 0.0)
    assert np.all(an["a"][0:3] != 0.0)
    assert np.linalg.norm(an["a"][0:3] - a_true[0:3]) < 0.5 * np.linalg.norm(a_true[0:3])
    assert an["err"][-1] < fd["err"][-1]


# ---------------------------------------------------------------------------
# 7. robust does its job
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("na", [6, 9])
def test_robust_resection_ends_closer_to_the_true_pose(gpu, na):
    P, a_true = _cam(513, 700 + na, na)
    P = dict(P)
    P["obs_x"], out = rr.plant_outliers(P["obs_x"], seed=na)
    assert 8 <= out.sum() <= 30
    dist = lambda a: float(np.linalg.norm(a[0:6] - a_true[0:6]))
    kw = dict(stop_rel=1e-9, max_iter=100, max_iter2=20)
    ref = {k: br.block_lm(P, k, 3.0, **kw)[0] for k in ("none", "huber", "cauchy")}
    assert dist(ref["huber"]) < dist(ref["none"]) and dist(ref["cauchy"]) < dist(ref["none"])
    (plain,), _ = _resect(gpu, [P], na, jacobian="analytic", **kw)
    for kind in ("huber", "cauchy"):
        (r,), _ = _resect(gpu, [P], na, jacobian="analytic", loss=kind, loss_scale=3.0, **kw)
        print(f"na {na} {kind}: pose error {dist(r['a']):.4g} (plain {dist(plain['a']):.4g}; "
              f"reference {dist(ref[kind]):.4g} / {dist(ref['none']):.4g}); outlier weights <= "
              f"{r['w'][out].max():.3g}; {int((r['w'] < 1).sum())} weights below 1")
        assert dist(r["a"]) < dist(plain["a"])
        assert np.all(r["w"][out] < 1.0)
        if kind == "huber":      # exactly the observations beyond the scale
            s = (r["e"] ** 2).sum(1)
            assert np.array_equal(r["w"] < 1.0, s > 9.0)
    assert np.all(plain["w"] == 1.0)


# ---------------------------------------------------------------------------
# 8. triangulation under the lens
# ---------------------------------------------------------------------------
def _undistorted(s):
    x = np.zeros_like(s["x"])
    for o in range(len(x)):
        j = s["cam"][o]
        u = br.undistort_mp(s["K"][0, j], s["K"][2:4, j], s["kd"][0, j], s["kd"][1, j], s["x"][o])
        assert u is not None
        x[o] = u
    return x


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_triangulation_under_the_lens(gpu, n):
    s = _tracks(n, True)
    X, st = gpu.triangulate_points(s["K"], s["T"], s["w"], s["ptr"], s["cam"], s["x"],
                                   radial=s["kd"], return_status=True)
    nv = np.diff(s["ptr"])
    xu = _undistorted(s)
    Kf = s["K"].copy()
    Kf[1] = Kf[0]
    Xs, sr = tr.triangulate_ref(Kf, s["T"], s["w"], s["ptr"], s["cam"], xu)
    assert np.array_equal(st, sr) and np.all(st[nv < 2] == 2) and np.all(st[nv >= 2] == 1)
    assert np.all(X[:, st != 1] == 0.0)
    ok = np.nonzero(st == 1)[0]        # the 60-digit reference on every triangulated point
    assert len(ok) == (nv >= 2).sum()
    if len(ok):
        cl = [s["cam"][s["ptr"][i]:s["ptr"][i + 1]] for i in ok]
        xl = [xu[s["ptr"][i]:s["ptr"][i + 1]] for i in ok]
        Xm = tr.triangulate_mp(Kf, s["T"], s["w"], *tr.pack(cl, xl))
        e_gpu, e_svd = tr.rel_err(X[:, ok], Xm), tr.rel_err(Xs[:, ok], Xm)
        print(f"n {n}: gpu {e_gpu:.3e}  numpy svd {e_svd:.3e}  ratio {e_gpu / e_svd:.3f}")
        assert e_gpu <= 16 * e_svd
    # the pinhole scene through a lens of all zeros agrees with vlgba_triangulate
    p = _tracks(n, False)
    X0, s0 = gpu.triangulate_points(p["K"], p["T"], p["w"], p["ptr"], p["cam"], p["x"],
                                    return_status=True)
    Xz, sz = gpu.triangulate_points(p["K"], p["T"], p["w"], p["ptr"], p["cam"], p["x"],
                                    radial=np.zeros((2, p["m"])), return_status=True)
    assert np.array_equal(s0, sz)
    ok = np.nonzero(s0 == 1)[0]
    if len(ok):             # the same bar: against the 60-digit reference, every point
        cl = [p["cam"][p["ptr"][i]:p["ptr"][i + 1]] for i in ok]
        xl = [p["x"][p["ptr"][i]:p["ptr"][i + 1]] for i in ok]
        csr = tr.pack(cl, xl)
        Xm = tr.triangulate_mp(p["K"], p["T"], p["w"], *csr)
        Xs, _ = tr.triangulate_ref(p["K"], p["T"], p["w"], *csr)
        e_zero, e_plain, e_svd = (tr.rel_err(q, Xm) for q in (Xz[:, ok], X0[:, ok], Xs))
        print(f"n {n} zero lens: {e_zero:.3e}  vlgba_triangulate {e_plain:.3e}  svd {e_svd:.3e}")
        assert e_zero <= 16 * e_svd and e_plain <= 16 * e_svd
        assert tr.rel_err(Xz[:, ok], X0[:, ok]) <= 1e-9


def test_triangulation_planted_failures(gpu):
    """a point behind a camera (status 0), and one observation past the fold of
    a strongly distorted lens (status 2, zeros); the others keep status 1"""
    s = dict(_tracks(10, True))
    kd = s["kd"].copy()
    kd[:, 3] = (-0.5, 0.0)       # r d(r) peaks at 0.5443: |nd| = 0.6 has no preimage
    K = s["K"]
    x = s["x"].copy()
    nv = np.diff(s["ptr"])
    full = np.nonzero(nv == 9)[0]
    o = s["ptr"][full[0]] + int(np.nonzero(s["cam"][s["ptr"][full[0]]:s["ptr"][full[0] + 1]]
                                           == 3)[0][0])
    x[o] = (K[2, 3] + 0.6 * K[0, 3], K[3, 3])
    assert br.undistort_mp(K[0, 3], K[2:4, 3], -0.5, 0.0, x[o]) is None
    X, st = gpu.triangulate_points(K, s["T"], s["w"], s["ptr"], s["cam"], x, radial=kd,
                                   return_status=True)
    assert st[full[0]] == 2 and np.all(X[:, full[0]] == 0.0)
    X1, s1 = gpu.triangulate_points(K, s["T"], s["w"], s["ptr"], s["cam"], s["x"], radial=kd,
                                    return_status=True)
    keep = np.arange(s["n"]) != full[0]
    assert s1[full[0]] == 1          # the same lens inverts the point's own measurement
    assert np.array_equal(st[keep], s1[keep]) and np.array_equal(X[:, keep], X1[:, keep])
    X1, s1 = gpu.triangulate_points(K, s["T"], s["w"], s["ptr"], s["cam"], s["x"],
                                    radial=s["kd"], return_status=True)
    # behind: a point on the far side of cameras 0 and 1, seen through the lens
    # formula at negative depth (the pixel of its mirror image)
    import jac_ref as jr
    R = np.asarray(jr.rodrigues(s["w"]), dtype=np.float64)
    C = [-R[:, :, j].T @ s["T"][:, j] for j in (0, 1)]
    Xb = 2.0 * (C[0] + C[1]) / 2
    xb = []
    for j in (0, 1):
        Xc = R[:, :, j] @ Xb + s["T"][:, j]
        assert Xc[2] < 0
        nn = Xc[:2] / Xc[2]
        r2 = nn @ nn
        xb.append(K[0, j] * (1 + rad.K_TRUE[0] * r2 + rad.K_TRUE[1] * r2 * r2) * nn + K[2:4, j])
    ptr = np.concatenate([s["ptr"], [s["ptr"][-1] + 2]])
    cam = np.concatenate([s["cam"], [0, 1]]).astype(np.int32)
    X2, s2 = gpu.triangulate_points(K, s["T"], s["w"], ptr, cam, np.vstack([s["x"], xb]),
                                    radial=s["kd"], return_status=True)
    print(f"planted: fold status {st[full[0]]}, point behind cameras 0 and 1 status {s2[-1]}")
    assert s2[-1] == 0 and np.all(X2[:, -1] == 0.0)
    assert np.array_equal(s2[:-1], s1) and np.array_equal(X2[:, :-1], X1)


# ---------------------------------------------------------------------------
# 9. arguments (with a device present)
# ---------------------------------------------------------------------------
def test_arguments(gpu):
    import test_block_ref as cpu
    assert cpu._resect_ex(na=9, jac=0) == cpu.E_ARG
    assert cpu._resect_ex(na=12) == cpu.E_NUMA
    assert cpu._resect_ex(loss=1, scale=0.0) == cpu.E_ARG
    assert cpu._resect_ex(nprob=0, ptr=(0,)) == 0
    assert cpu._call("intersect", cpu._args(), null=(), jac=0) == cpu.E_ARG
    assert cpu._call("intersect", cpu._args(n=0, ptr=(0,), cam=())) == 0
    assert cpu._call("triangulate", cpu._args(n=0, ptr=(0,), cam=()), null=()) == 0
    # NULL optional outputs on a real run; the plain entry still refuses num_a = 9
    P = _cam(6, 106, 9)[0]
    K = P["K"].copy()
    K[0] = P["a"][6]
    out = gpu.bundle_euclid_resect(K, P["a"][3:6], P["a"][0:3], [P["b"]], [P["obs_x"].T],
                                   radial=P["a"][7:9])
    assert len(out) == 5 and len(out[3][0]) >= 2 and out[4].shape == (2, 1)
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, VlgbaResectProblem, c_dp
    import ctypes
    ptr = np.array([0, 6], dtype=np.int64)
    X = np.ascontiguousarray(P["b"].T)
    a = P["a"][:, 0].copy()
    pr = VlgbaResectProblem(1, 9, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                            X.ctypes.data_as(c_dp), P["obs_x"].ctypes.data_as(c_dp),
                            K.ctypes.data_as(c_dp))
    assert gpu.lib().vlgba_resect(ctypes.byref(pr), ctypes.byref(VlgbaOptions()),
                                  a.ctypes.data_as(c_dp), None, 0, None, None) == cpu.E_NUMA
    s = _tracks(5, True)
    X_, errs = gpu.bundle_euclid_intersect(s["K"], s["T"], s["w"], s["X0"], s["ptr"], s["cam"],
                                           s["x"], radial=s["kd"])
    assert X_.shape == (3, 5) and len(errs[4]) >= 2
