"""GPU parity: libvlgba (HIP, gfx950) vs the CPU oracle restatement.

Tolerances (stated per test):
* stages 1-3 (projection, FD Jacobians, JtJ blocks, Schur complement, e_,
  back-substitution, update): BIT-EXACT (np.array_equal) -- same per-element
  expressions, same ascending summation order, -ffp-contract=off on both sides.
* reduced solve: Cholesky (GPU, MFMA blocked) vs LAPACK Cholesky / MATLAB-pinv
  (oracle): |da_gpu - da_ref| <= 1e-9 * |da_ref| (cond(S) ~ 1e6-1e8 here).
* whole LM: error_(1) within 1e-12 relative (tree vs BLAS summation of e'e);
  final cost inside the spread of the oracle's own variants (pinv vs Cholesky
  for S, SVD vs closed-form pinv for V*) widened by 1e-4 relative.  The
  reference's h = 1e-10 forward differences amplify rounding differences of da
  into ~1e-6 relative differences of the next Jacobians, so trajectories are
  chaotic at that level (config 1, fix_calibration: variants within 2e-5;
  free intrinsics: within 1e-2).  Points are compared through the cost they
  reproduce, which is invariant to the similarity gauge (see DESIGN.md "Parity").
"""
import numpy as np
import pytest

from conftest import random_problem

pytestmark = pytest.mark.gpu


def test_device_sincos_equals_libm(gpu, oracle):
    """The device sin / cos of the rotation tables (glibc's algorithm restated
    in vlg_libm.h, compiled for gfx950) equal the host libm bit for bit on 8M
    arguments over every branch of glibc's __sin / __cos -- the oracle's
    vl_rodrigues calls that libm."""
    import ctypes
    rng = np.random.default_rng(3)
    parts = [rng.uniform(lo, hi, 1_000_000) for lo, hi in
             [(0, 2.0 ** -26), (2.0 ** -26, 0.126), (0.126, 0.855469), (0.855469, 2.426265),
              (2.426265, 10.0), (10.0, 1e5), (0, 3.2), (1e-6, 1e-2)]]
    x = np.concatenate(parts)
    x = np.ascontiguousarray(x * rng.choice([-1.0, 1.0], x.size))
    s, c = np.empty_like(x), np.empty_like(x)
    rc = gpu.lib().vlgba_debug_sincos(x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.size)
    assert rc == 0
    s0, c0 = np.empty_like(x), np.empty_like(x)
    oracle._lib().oracle_libm_sincos(oracle.P(x), oracle.P(s0), oracle.P(c0),
                                     ctypes.c_longlong(x.size))
    bad = (s.view(np.int64) != s0.view(np.int64)) | (c.view(np.int64) != c0.view(np.int64))
    assert not bad.any(), (int(bad.sum()), x[bad][:5])


@pytest.mark.parametrize("num_a", [6, 7, 10])
@pytest.mark.parametrize("seed", [11, 12])
def test_stage1_bit_exact(gpu, oracle, num_a, seed):
    K, a, b, X, vis, _ = random_problem(seed, num_a=num_a)
    ref = oracle.mex1(K, a, b, X, vis)
    got = gpu.mex_bundle_1_XABeUVWeAeB(K, a, b, X, vis)
    names = "X_hat A B e U V W eA eB".split()
    for nm, r, g in zip(names, ref, got):
        assert r.shape == g.shape, nm
        assert np.array_equal(r, g), (nm, np.max(np.abs(r - g)))
    # camera 0 has w = 0: its rotation columns are exactly zero (App. A Q2)
    A = got[1]
    assert np.all(A[:, 0:3, :, 0] == 0.0)


@pytest.mark.parametrize("num_a", [6, 10])
def test_stage2_bit_exact(gpu, oracle, num_a):
    K, a, b, X, vis, _ = random_problem(21, num_a=num_a)
    _, _, _, _, U, V, W, eA, eB = oracle.mex1(K, a, b, X, vis)
    lam = 1e-3
    Us = U.copy(order="F")
    for k in range(num_a):
        Us[k, k] = (1 + lam) * U[k, k]
    Vs = V.copy(order="F")
    for k in range(3):
        Vs[k, k] = (1 + lam) * V[k, k]
    Vinv = oracle.pinv3_formula(Vs)
    Y = oracle.y_dense(W, Vinv)
    S_ref, e_ref = oracle.mex2(Y, W, Us, eA, eB)
    S, e_ = gpu.mex_bundle_2_Se_(Y, W, Us, eA, eB)
    assert np.array_equal(S, S_ref), np.max(np.abs(S - S_ref))
    assert np.array_equal(e_, e_ref), np.max(np.abs(e_ - e_ref))


@pytest.mark.parametrize("num_a", [6, 7, 10])
def test_stage3_bit_exact(gpu, oracle, num_a):
    K, a, b, X, vis, _ = random_problem(31, num_a=num_a)
    _, _, _, _, U, V, W, eA, eB = oracle.mex1(K, a, b, X, vis)
    Vinv = oracle.pinv3_formula(V + 0.1 * np.eye(3)[:, :, None] * V.max())
    rng = np.random.default_rng(5)
    da = rng.normal(0, 1e-4, (num_a * a.shape[1], 1))
    ref = oracle.mex3(W, da, eB, Vinv, K, a, b, X, vis)
    got = gpu.mex_bundle_3_db_new(W, da, eB, Vinv, K, a, b, X, vis)
    for nm, r, g in zip("db a_new b_new X_hat".split(), ref, got):
        assert np.array_equal(r, g), (nm, np.max(np.abs(r - g)))


def _final_cost(oracle, sc, res, vis, nvk):
    """Cost of the returned parameters, re-evaluated by the oracle (gauge-invariant)."""
    K_, Te_, w_, Xe_ = res[:4]
    a = oracle.pack_a(K_, Te_, w_, nvk)
    pt, cam, _ = oracle.obs_from_visibility(vis)
    x, _ = sc.dense()
    obs_x = np.stack([x[0, pt, cam], x[1, pt, cam]], 1)
    pb = oracle.SparseProblem(sc.m, sc.n, pt, cam, obs_x, K_ if nvk else sc.K)
    L = oracle.sp_linearize(pb, a, np.asfortranarray(Xe_[:3]), 6 + nvk)
    return float(L["e"].reshape(-1) @ L["e"].reshape(-1)) / vis.sum()


VARIANTS = [("pinv", "pinv"), ("pinv", "chol"), ("formula", "chol"), ("formula", "pinv")]


def _lm_compare(gpu, oracle, sc, opts, final_rtol=1e-4):
    """GPU LM vs the oracle.  The first error_ entry must agree to summation
    order; the final cost must lie inside the spread of the oracle's own
    variants (MATLAB pinv vs Cholesky for S, SVD pinv vs closed form for V*)
    widened by final_rtol -- the reference's FD Jacobians make the trajectory
    chaotic at that level, most of all with free intrinsics (measured spread
    3e-3 / 9e-3 relative for fix_principal / variable K on this scene)."""
    x, vis = sc.dense()
    res = gpu.bundle_euclid(sc.K, sc.T0, sc.w0, sc.X0, x, "visibility", vis, *opts)
    finals, refs = [], []
    for vinv, solve in VARIANTS:
        r = oracle.bundle_euclid_ref(sc.K, sc.T0, sc.w0, sc.X0, x, "visibility", vis, *opts,
                                     form="sparse", vinv=vinv, solve=solve)
        refs.append(r)
        if len(r[4]):
            finals.append(r[4][-1])
    err = res[4]
    assert (len(err) == 0) == (len(finals) == 0)
    if len(err):
        e0 = refs[0][4][0]
        assert abs(err[0] - e0) <= 1e-12 * abs(e0)
        # first accepted step: same linearisation, da equal to rounding
        e1 = [r[4][1] for r in refs if len(r[4]) > 1]
        assert min(e1) * (1 - 1e-7) <= err[1] <= max(e1) * (1 + 1e-7), (err, e1)
        assert np.all(np.diff(err) <= 0)                 # error_ never increases
        lo, hi = min(finals), max(finals)
        assert lo * (1 - final_rtol) <= err[-1] <= hi * (1 + final_rtol), (err, finals)
        nvk = 0 if "fix_calibration" in opts else (1 if "fix_principal" in opts else 4)
        # the returned parameters reproduce the reported cost (gauge-invariant)
        assert abs(_final_cost(oracle, sc, res, vis, nvk) - err[-1]) <= 1e-9 * err[-1]
    return res, refs


def test_lm_config1(gpu, oracle):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg1")
    res, refs = _lm_compare(gpu, oracle, sc, ("fix_calibration",))
    # fix_calibration: every variant within 1e-4 of the reference semantics
    assert abs(res[4][-1] - refs[0][4][-1]) <= 1e-4 * refs[0][4][-1]
    assert len(res[4]) == len(refs[0][4])


@pytest.mark.parametrize("opts,rtol", [(("fix_principal",), 3e-2), ((), 3e-2),
                                       (("fix_calibration", "fix_structure"), 1e-4),
                                       (("fix_calibration", "fix_motion"), 1e-4)])
def test_lm_options(gpu, oracle, opts, rtol):
    """Free intrinsics make the reference's own trajectory chaotic (its pinv /
    Cholesky variants end 0.3-0.9 % apart and stop after 3-6 steps), so the
    final cost is bounded by the variants' spread widened by 3 %; the first
    step must still agree to rounding (checked in _lm_compare)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg1", m=6, min_n=30, max_n=60, seed=7)
    _lm_compare(gpu, oracle, sc, opts, final_rtol=rtol)


def test_lm_fix_pivot(gpu, oracle):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg1", m=6, min_n=30, max_n=60, seed=8)
    pivot = np.zeros(sc.m, dtype=bool)
    pivot[[0, 1]] = True
    res, _ = _lm_compare(gpu, oracle, sc, ("fix_calibration", "fix_pivot", pivot),
                         final_rtol=1e-4)
    # pivot cameras are not moved
    assert np.array_equal(res[2][:, :2], sc.w0[:, :2])
    assert np.array_equal(res[1][:, :2], sc.T0[:, :2])


@pytest.mark.parametrize("opts,final_rtol", [(("fix_calibration",), 1e-4), ((), 3e-2)])
def test_lm_nomex_semantics(gpu, oracle, opts, final_rtol):
    """bundle_euclid_nomex (the pure-MATLAB twin's semantics: full-da back
    substitution, no fix_pivot, Xe_(4,:) = 1) vs the oracle with the same
    semantics: first error_ entry to summation order, first accepted step to
    rounding, final cost inside the oracle variants' spread."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg1", m=6, min_n=30, max_n=60, seed=7)
    x, vis = sc.dense()
    pv = np.zeros(sc.m, dtype=bool)
    pv[:2] = True
    res = gpu.bundle_euclid_nomex(sc.K, sc.T0, sc.w0, sc.X0, x, "visibility", vis, *opts,
                                  "fix_pivot", pv)                 # ignored by the twin
    refs = [oracle.bundle_euclid_ref(sc.K, sc.T0, sc.w0, sc.X0, x, "visibility", vis, *opts,
                                     form="sparse", vinv=vinv, solve=solve, semantics="nomex")
            for vinv, solve in VARIANTS]
    err = res[4]
    assert abs(err[0] - refs[0][4][0]) <= 1e-12 * refs[0][4][0]
    e1 = [r[4][1] for r in refs]
    assert min(e1) * (1 - 1e-7) <= err[1] <= max(e1) * (1 + 1e-7), (err, e1)
    finals = [r[4][-1] for r in refs]
    assert min(finals) * (1 - final_rtol) <= err[-1] <= max(finals) * (1 + final_rtol)
    assert np.all(res[3][3] == 1.0)
    assert not np.array_equal(res[2][:, :2], sc.w0[:, :2])      # pivot cameras moved


def test_envelope_equals_dense_solve(gpu):
    """Skipping the tiles outside the envelope of S is exact: every result of a
    pass is bit-identical to factoring all lower tiles (sequential tile
    Cholesky both times; the default solver would use cyclic reduction here)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=40, n=4000, seed=12)
    a = np.zeros((6, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    out = []
    for solver in ("envelope", "dense"):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, solver=solver)
        ba.set_params(a, b)
        infos = [ba.step(relinearize=True, update_lm=True) for _ in range(3)]
        out.append(([(i.old_sse, i.new_sse, i.dpg) for i in infos], ba.get_params()))
        ba.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1][0], out[1][1][0]) and np.array_equal(out[0][1][1],
                                                                          out[1][1][1])


@pytest.mark.parametrize("num_a", [6, 7, 10])
@pytest.mark.parametrize("cfg", ["cfg2", "cfg5"])
def test_linearization_bit_exact(gpu, oracle, num_a, cfg):
    """Stage 1 through the handle API: the chunked fast path (two lanes per
    observation, shared-reciprocal / Markstein divisions, LDS-staged A, B, e)
    and the ordered path both give W, V, eB bit-identical to the oracle; U, eA
    are bit-identical in ordered mode and equal to summation-grouping rounding
    in fast mode (per-chunk partials)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config(cfg, seed=17) if cfg == "cfg2" else make_config(cfg, m=12, seed=17)
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    b = np.asfortranarray(sc.X0[:3])
    a[0, 1], a[1, 1] = -0.0, 0.0   # R(w + 0 h) != R(w) bitwise when a zero of w is -0
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    ref = oracle.sp_linearize(pb, a, b, num_a)
    for ordered in (False, True):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a,
                                ordered=ordered)
        ba.set_params(a, b)
        got = ba.linearization()
        ba.close()
        W = got["W"].reshape(3 * num_a, -1, order="F").T
        assert np.array_equal(W, ref["W"]), np.max(np.abs(W - ref["W"]))
        assert np.array_equal(got["V"], ref["V"])
        assert np.array_equal(got["eB"], ref["eB"])
        for nm in ("U", "eA"):
            if ordered:
                assert np.array_equal(got[nm], ref[nm]), nm
            else:
                scale = np.max(np.abs(ref[nm]))
                assert np.max(np.abs(got[nm] - ref[nm])) <= 1e-13 * scale, nm


def _one_pass(gpu, sc, num_a, **kw):
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    b = np.asfortranarray(sc.X0[:3])
    ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, **kw)
    ba.set_params(a, b)
    ba.set_timing(True)
    info = ba.step(relinearize=True, update_lm=False)
    km = ba.kernel_ms()
    ba.close()
    return info, km


@pytest.mark.parametrize("num_a,m", [(6, 200), (6, 11), (7, 75), (10, 64)])
def test_cyclic_reduction_matches_envelope(gpu, num_a, m):
    """Banded co-visibility (tile-tridiagonal S): the default solver runs block
    cyclic reduction (log2 levels) and agrees with the sequential envelope
    Cholesky to rounding; odd / even / power-of-two tile counts.  (Two pass
    scalars only: tests/test_gpu_cr_branches.py holds every entry of da on
    this route -- the 64-row reduction at num_a 6 / 7 / 9 / 10 / 12, split and
    unsplit bodies -- to the long double solve reference.)"""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=m, n=60 * m, seed=31)
    cr, kcr = _one_pass(gpu, sc, num_a)
    env, kenv = _one_pass(gpu, sc, num_a, solver="envelope")
    # 6-camera tracks: camera-aligned 32-row tiles for num_a = 6 (groups of 5
    # cameras), 64-row tiles otherwise
    rows = num_a * (32 // num_a) if num_a == 6 else 64
    nt = -(-num_a * m // rows)
    assert "k_cr_factor" in kcr and "k_factor_step" not in kcr
    # levels: floor(log2 nt) + 1 launches, or ONE (k_cr32_fused) for the
    # camera-aligned tiles
    assert kcr["k_cr_factor"][1] == (1 if rows <= 32 else nt.bit_length())
    assert "k_factor_step" in kenv and "k_cr_factor" not in kenv
    assert cr.old_sse == env.old_sse
    assert cr.chol_failed == 0 and env.chol_failed == 0
    assert abs(cr.new_sse - env.new_sse) <= 1e-9 * env.new_sse, (cr.new_sse, env.new_sse)
    assert abs(cr.dpg - env.dpg) <= 1e-9 * abs(env.dpg), (cr.dpg, env.dpg)


@pytest.mark.parametrize("num_a", [6, 7, 10])
def test_fast_path_matches_ordered(gpu, num_a):
    """Chunked linearisation + fused Schur path vs the ordered (bit-exact)
    kernels: W, V, eB identical; U, eA, SSE, the reduced system and the step
    equal to summation-order rounding (chunk partials)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=30, n=3000, seed=13)
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    b = np.asfortranarray(sc.X0[:3])
    res, plans = [], []
    for ordered, kern in ((True, "auto"), (False, "terms"), (False, "auto")):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a,
                                ordered=ordered, schur_kernel=kern)
        ba.set_params(a, b)
        info = ba.step(relinearize=True, update_lm=False)
        res.append(info)
        plans.append(ba.plan_info())
        ba.close()
    assert [p["mfma"] for p in plans] == [0, 0, 1]
    o = res[0]
    for f in res[1:]:
        assert abs(o.old_sse - f.old_sse) <= 1e-13 * o.old_sse, (o.old_sse, f.old_sse)
        assert abs(o.new_sse - f.new_sse) <= 1e-8 * o.new_sse, (o.new_sse, f.new_sse)
        assert abs(o.dpg - f.dpg) <= 1e-8 * abs(o.dpg), (o.dpg, f.dpg)


@pytest.mark.parametrize("seed", [1, 2])
def test_mfma_schur_on_banded_scene(gpu, seed):
    """Video-like banded tracks (config-3 shape, scaled down): the MFMA Schur
    chunks and the per-term kernel give the same reduced system to rounding,
    on accepted and rejected (re-damped, no relinearisation) passes."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg3", m=120, n=30000, seed=seed)
    a = np.zeros((6, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    out = {}
    for kern in ("terms", "auto"):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6,
                                schur_kernel=kern)
        ba.set_params(a, b)
        i1 = ba.step(relinearize=True, update_lm=False)
        i2 = ba.step(relinearize=False, update_lm=False)
        out[kern] = (i1, i2, ba.plan_info()["mfma"])
        ba.close()
    assert out["terms"][2] == 0 and out["auto"][2] == 1
    for t, f in zip(out["terms"][:2], out["auto"][:2]):
        # SSE partials are summed per chunk, and the two plans chunk differently
        assert abs(t.old_sse - f.old_sse) <= 1e-13 * t.old_sse, (t.old_sse, f.old_sse)
        assert abs(t.new_sse - f.new_sse) <= 1e-9 * t.new_sse, (t.new_sse, f.new_sse)
        assert abs(t.dpg - f.dpg) <= 1e-9 * abs(t.dpg), (t.dpg, f.dpg)


def test_single_pass_config2(gpu, oracle):
    """One full LM pass at config-2 size: linearisation bit-exact (old SSE to
    summation order), da vs LAPACK Cholesky within 1e-9 relative."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2")
    num_a = 6
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    L = oracle.sp_linearize(pb, a, b, num_a)
    lam = 1e-3
    Us = L["U"].copy(order="F")
    for k in range(num_a):
        Us[k, k] = (1 + lam) * L["U"][k, k]
    Vs = L["V"].copy(order="F")
    for k in range(3):
        Vs[k, k] = (1 + lam) * L["V"][k, k]
    Vinv = oracle.pinv3_formula(Vs)
    Y = oracle.sp_y(pb, L["W"], Vinv, num_a)
    S, e_ = oracle.sp_schur(pb, Y, L["W"], Us, L["eA"], L["eB"], num_a)
    da = oracle.chol_solve_fixed(S, e_)
    db, a_new, b_new, xh, sse = oracle.sp_update(pb, L["W"], da, L["eB"], Vinv, a, b, num_a)
    old = float(L["e"].reshape(-1) @ L["e"].reshape(-1))
    ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a)
    ba.set_params(a, b)
    info = ba.step(relinearize=True, update_lm=False)
    assert abs(info.old_sse - old) <= 1e-12 * old
    assert abs(info.new_sse - sse) <= 1e-7 * sse, (info.new_sse, sse)
    ba.close()


@pytest.mark.parametrize("num_a,track,rows", [(7, 5, 28), (10, 4, 30), (12, 3, 24)])
def test_cyclic_reduction_tile_heights(gpu, num_a, track, rows):
    """Camera-aligned cyclic-reduction tiles of NA * floor(32 / NA) rows for
    num_a = 7 / 10 and the projective camera (12): tracks of G + 1 consecutive
    cameras keep S tridiagonal in G-camera tiles.  The fused level kernel's
    fill / survivor records for these heights agree with the envelope
    Cholesky to rounding."""
    from bundleadjustmentmatlab_amd.scene import make_config, projective_from
    m = 90
    sc = make_config("cfg2", m=m, n=40 * m, track=track, seed=41)
    if num_a == 12:
        Pp, Xp = projective_from(sc)
        a = np.asfortranarray(Pp.reshape(12, m, order="F"))
        b = np.asfortranarray(Xp[0:3])
        kw = dict(model="projective", m=m)
        K = None
    else:
        a = np.zeros((num_a, m), order="F")
        a[0:3], a[3:6] = sc.w0, sc.T0
        if num_a == 7:
            a[6] = sc.K[0]
        else:
            a[6:10] = sc.K
        b = np.asfortranarray(sc.X0[:3])
        kw = {}
        K = sc.K
    out = {}
    for solver in ("auto", "envelope"):
        ba = gpu.BundleAdjuster(K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, solver=solver,
                                **kw)
        ba.set_params(a, b)
        info = ba.step(relinearize=True, update_lm=False)
        out[solver] = (info, ba.plan_info())
        ba.close()
    assert out["auto"][1]["cr_rows"] == rows
    assert out["envelope"][1]["cr_levels"] == 0
    cr, env = out["auto"][0], out["envelope"][0]
    assert cr.chol_failed == 0 and env.chol_failed == 0
    assert cr.old_sse == env.old_sse
    assert abs(cr.new_sse - env.new_sse) <= 1e-9 * env.new_sse, (cr.new_sse, env.new_sse)
    assert abs(cr.dpg - env.dpg) <= 1e-9 * abs(env.dpg), (cr.dpg, env.dpg)


def test_run_error_capacity(gpu):
    """error_ is sized from max_iter (a 64-entry buffer used to be
    passed whatever max_iter was); the library clamps to the capacity given."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=20, n=1500, seed=4)
    a = np.zeros((6, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, max_iter=100,
                            max_iter2=30)
    ba.set_params(a, b)
    err, st = ba.run()
    assert len(err) == st.num_error <= 100 and np.all(np.isfinite(err))
    # an explicit small capacity: only the first entries are written
    import ctypes
    ba.set_params(a, b)
    buf = np.full(4, -1.0)
    st2 = gpu._lib.VlgbaStats()
    rc = gpu.lib().vlgba_run(ba._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 2,
                             ctypes.byref(st2))
    ba.close()
    assert rc == 0 and st2.num_error == st.num_error
    assert np.array_equal(buf[:2], err[:2]) and np.all(buf[2:] == -1.0)


@pytest.mark.parametrize("num_a", [6, 7])
def test_mixed_mfma_and_term_chunks(gpu, oracle, num_a):
    """Irregular tracks (ladybug-like: 2..30 views, loop closures): the short
    tracks run in MFMA Schur chunks and the long ones in per-term chunks in one
    plan (points reordered internally, short tracks first).  One pass matches
    the ordered kernels and the terms-only plan to summation-order rounding;
    the stage-1 getters and the accepted parameters come back in the input
    point / observation order (W, V, eB bit-identical to the oracle)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("ladybug", m=80, n=4000, max_track=30, radius=150.0, seed=23)
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    b = np.asfortranarray(sc.X0[:3])
    res = {}
    for name, kw in (("ordered", dict(ordered=True)), ("terms", dict(schur_kernel="terms")),
                     ("mixed", {})):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, **kw)
        ba.set_params(a, b)
        lin = ba.linearization() if name == "mixed" else None
        info = ba.step(relinearize=True, update_lm=True)
        a2, b2 = ba.get_params()
        da, db = ba.last_step()
        res[name] = (info, ba.plan_info(), a2, b2, db, lin)
        ba.close()
    pl = res["mixed"][1]
    assert 0 < pl["mfma_groups"] < pl["groups"] and pl["reordered"] == 1
    assert res["terms"][1]["mfma_groups"] == 0 and res["terms"][1]["reordered"] == 0
    o = res["ordered"]
    for nm in ("terms", "mixed"):
        f = res[nm]
        assert abs(o[0].old_sse - f[0].old_sse) <= 1e-13 * o[0].old_sse
        assert abs(o[0].new_sse - f[0].new_sse) <= 1e-8 * o[0].new_sse, nm
        assert abs(o[0].dpg - f[0].dpg) <= 1e-8 * abs(o[0].dpg), nm
        assert o[0].accepted == f[0].accepted == 1
        assert np.max(np.abs(f[3] - o[3])) <= 1e-8 * np.max(np.abs(o[3]))   # b_new
        assert np.max(np.abs(f[4] - o[4])) <= 1e-6 * np.max(np.abs(o[4]))   # db
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    ref = oracle.sp_linearize(pb, a, b, num_a)
    lin = res["mixed"][5]
    assert np.array_equal(lin["W"].reshape(3 * num_a, -1, order="F").T, ref["W"])
    assert np.array_equal(lin["V"], ref["V"]) and np.array_equal(lin["eB"], ref["eB"])


@pytest.mark.parametrize("kern", ["auto", "terms"])
def test_long_tracks_fast_path(gpu, oracle, kern):
    """Tracks longer than a Schur chunk holds (here 100-216 views, > 128 and
    > 90) no longer switch the whole problem to the ordered kernels: they are
    split into segment chunks (segmented V / eB sums), their (obs, obs) terms
    run in the long-track tiles and their db over all their observations.  One
    pass matches the ordered kernels to summation-order rounding; V / eB of
    the long tracks to 1e-13 (segment sums), W and the rest bit-exact."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("ladybug", m=300, n=5000, max_track=30, radius=150.0, seed=29,
                     long_frac=0.01, long_len=(100, 220))
    L = np.bincount(sc.obs_pt, minlength=sc.n)
    assert (L > 128).sum() > 10
    num_a = 6
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    b = np.asfortranarray(sc.X0[:3])
    res = {}
    for name, kw in (("ordered", dict(ordered=True)), ("fast", dict(schur_kernel=kern))):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, **kw)
        ba.set_params(a, b)
        lin = ba.linearization()
        i1 = ba.step(relinearize=True, update_lm=False)
        db1 = ba.last_step()[1]
        # the same linearisation again (no relinearisation: the long tracks'
        # V sums, V*^-1 and tiles from the kept stage-1 outputs)
        i2 = ba.step(relinearize=False, update_lm=False)
        res[name] = (i1, i2, ba.plan_info(), db1, ba.last_step()[1], lin)
        ba.close()
    pl = res["fast"][2]
    assert pl["ordered"] == 0 and pl["long_points"] == (L > 128).sum() + ((L <= 128) & (L * (L + 1) // 2 > 4096)).sum()
    o, f = res["ordered"], res["fast"]
    for io, jf in ((o[0], f[0]), (o[1], f[1])):
        assert abs(io.old_sse - jf.old_sse) <= 1e-12 * io.old_sse
        assert abs(io.new_sse - jf.new_sse) <= 1e-8 * io.new_sse, (io.new_sse, jf.new_sse)
        assert abs(io.dpg - jf.dpg) <= 1e-8 * abs(io.dpg), (io.dpg, jf.dpg)
        assert io.accepted == jf.accepted
    # (a second relinearised pass would differ at the FD noise floor, ~1e-6:
    # the Jacobians at points one rounding apart)
    for q in (3, 4):
        assert np.max(np.abs(f[q] - o[q])) <= 1e-8 * np.max(np.abs(o[q]))
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    ref = oracle.sp_linearize(pb, a, b, num_a)
    lin = f[5]
    assert np.array_equal(lin["W"].reshape(3 * num_a, -1, order="F").T, ref["W"])
    for nm in ("V", "eB"):
        assert np.allclose(lin[nm], ref[nm], rtol=1e-13, atol=1e-13 * np.abs(ref[nm]).max()), nm
    for nm in ("U", "eA"):
        assert np.max(np.abs(lin[nm] - ref[nm])) <= 1e-13 * np.max(np.abs(ref[nm])), nm


def _cr_pass(gpu, sc, num_a, fused, **kw):
    """One LM pass with the one-launch CR (k_cr32_fused) or the per-level
    launches (VLGBA_CR_FUSED=0, read when the context is set up): pass info,
    kernel timers, the step (da, db)."""
    import os
    old = os.environ.get("VLGBA_CR_FUSED")
    os.environ["VLGBA_CR_FUSED"] = "1" if fused else "0"
    try:
        a = np.zeros((num_a, sc.m), order="F")
        a[0:3], a[3:6] = sc.w0, sc.T0
        if num_a == 7:
            a[6] = sc.K[0]
        elif num_a == 10:
            a[6:10] = sc.K
        b = np.asfortranarray(sc.X0[:3])
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, **kw)
        ba.set_params(a, b)
        ba.set_timing(True)
        info = ba.step(relinearize=True, update_lm=False)
        km = ba.kernel_ms()
        da, db = ba.last_step()
        plan = ba.plan_info()
        ba.close()
    finally:
        if old is None:
            del os.environ["VLGBA_CR_FUSED"]
        else:
            os.environ["VLGBA_CR_FUSED"] = old
    return info, km, np.array(da, copy=True), np.array(db, copy=True), plan


def test_cr_back_substitution_one_launch_and_fallback(gpu):
    """Per-level CR launches (VLGBA_CR_FUSED=0): the back substitution runs as
    one launch with in-kernel hand-offs while every elimination record is
    co-resident (<= 2 x CUs), and as one launch per level beyond; both agree
    with the envelope Cholesky."""
    from bundleadjustmentmatlab_amd.scene import make_config
    for m, launches in ((200, 1), (3000, None)):
        sc = make_config("cfg2", m=m, n=10 * m, seed=37)
        cr, kcr, _, _, _ = _cr_pass(gpu, sc, 6, fused=False)
        env, _ = _one_pass(gpu, sc, 6, solver="envelope")
        nrec = -(-6 * m // 30)                          # 30-row camera-aligned tiles
        calls = kcr["k_cr_back"][1]
        if launches is not None:
            assert calls == launches
        else:                                           # more records than 2 x CUs
            assert calls == nrec.bit_length() and nrec > 2 * 256
        assert cr.chol_failed == 0
        assert abs(cr.new_sse - env.new_sse) <= 1e-9 * env.new_sse, (m, cr.new_sse, env.new_sse)
        assert abs(cr.dpg - env.dpg) <= 1e-9 * abs(env.dpg), (m, cr.dpg, env.dpg)


@pytest.mark.parametrize("num_a,m,track", [(6, 200, 6), (6, 11, 6), (6, 3000, 6), (6, 6, 2),
                                           (7, 75, 5), (10, 64, 4)])
def test_cr_one_launch_bit_identical(gpu, num_a, m, track):
    """The whole cyclic reduction in ONE launch (k_cr32_fused: factor levels
    and back substitution as records with in-kernel hand-offs) performs the
    per-level kernels' arithmetic record for record: the step da / db and the
    pass scalars are bit-identical to the per-level launches', for odd / even /
    power-of-two tile counts, tile heights 30 / 28, and more records than
    CUs (m = 3000: 600 tiles, ~2000 records on 256 CUs at one per CU)."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=m, n=max(40, 10 * m), track=track, seed=43 + m)
    f_info, f_km, f_da, f_db, plan = _cr_pass(gpu, sc, num_a, fused=True)
    l_info, l_km, l_da, l_db, _ = _cr_pass(gpu, sc, num_a, fused=False)
    assert plan["cr_levels"] > 0 and plan["cr_rows"] > 0
    assert f_km["k_cr_factor"][1] == 1 and "k_cr_back" not in {k for k, v in f_km.items()
                                                                if v[1] > 0}
    assert l_km["k_cr_factor"][1] == plan["cr_levels"]
    assert f_info.chol_failed == 0 and l_info.chol_failed == 0
    assert np.array_equal(f_da, l_da)
    assert np.array_equal(f_db, l_db)
    assert f_info.new_sse == l_info.new_sse and f_info.dpg == l_info.dpg
