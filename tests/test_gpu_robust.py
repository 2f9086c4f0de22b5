"""Robust losses (Huber, Cauchy) on the fast path (vlgba_set_loss, DESIGN.md
sec. 5) against tests/robust_ref.py, which tests/test_robust_ref.py proves on
the CPU.

1. Bit identity: Huber at scale 1e150 (c^2 = 1e300 above every s) takes every
   robust code path -- the LOSS instantiations of k_linearize_chunk,
   k_update_linearize and k_point_update_chunk, regular and segment chunks --
   with sqrt(w) == 1.0 and rho == s, so the whole run() equals the loss-none
   run bit for bit (error_, a, b, the stats): num_a 6 / 7 / 10 / 12, fused and
   VLGBA_FUSED=0, the long-track scene.  And set_loss("none") on a context that
   ran with a loss gives a fresh context's run again.
2. Stage: with ~3 % of the observations displaced by 30 .. 100 px and the scale
   at 3 px, linearization()'s U, eA, V, eB, W lie within robust_ref's per-entry
   bounds of the long double weighted sums of the oracle's A_o, B_o, e_o;
   residuals() has e bit-equal to the stage entry's x - x_hat, w and rho
   within their bounds; step().old_sse equals sum rho within the bound of an
   N-term sum; pivot cameras and fix_structure keep their exact zeros.
3. Fused against VLGBA_FUSED=0 with a loss: the applied step and the new
   linearisation bit-identical, the scalars to summation order, as
   tests/test_gpu_fused.py shows without a loss.
4. The solvers: cyclic reduction (banded), nested dissection / envelope
   (ladybug), and a forced pinv pass that still lowers the robust cost.
5. Converged cost: robust_lm started at the GPU's converged parameters lowers
   the robust cost by at most 1e-6 relative (the restart criterion of
   tests/test_gpu_converged.py).
6. End to end on the planted-outlier scene: the conditions robust_ref.e2e_check
   states, which the reference meets on the CPU.
7. Arguments.   8. Two rank threads against one rank.

Every test prints its figures before it asserts (lines starting ROBUST, pytest -s).
Measured on an MI355X; no bar was widened.  Largest |diff| / bound of the stage
check over all its cases: U 0.073, eA 0.11, V 0.15, eB 0.15, W 0.25, w 0.23,
rho 0.36, the cost 0.001 (Huber and Cauchy alike; the largest U and eA on the
140-camera point).  The ladders of tests/track_scenes.py (tracks of up to 257 /
273 / 280 views in three segments, num_a 7 / 10 / 12, Huber): U 0.10, eA 0.070,
V 0.11, eB 0.14, W 0.22, w 0.21, rho 0.23, the cost 0.0002.  Converged Cauchy cost 1.871022836, the reference's robust LM
from there 1.871022758 (drop 4.2e-8).  End to end: inlier RMS 4.9 px after the
plain solve, 0.61 px after the Cauchy solve; largest weight of a planted outlier
0.0098; every inlier above 0.5 (the reference on the CPU: 4.895, 0.6143, 0.0098,
every inlier).
"""
import functools
import os

import numpy as np
import pytest

import robust_ref as rr

pytestmark = pytest.mark.gpu

TRACK = {6: 6, 7: 5, 10: 4, 12: 3}          # as tests/test_gpu_stage_ref.py
CAMS = {6: 33, 7: 33, 10: 34, 12: 33}
SCALE = 3.0
STOP = dict(stop_rel=1e-12, max_iter=200, max_iter2=30)   # tests/test_gpu_converged.py


@functools.lru_cache(maxsize=None)
def _banded(na):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=CAMS[na], n=1327, track=TRACK[na], seed=41)
    return sc, sc.obs_pt, sc.obs_cam, sc.obs_x


@functools.lru_cache(maxsize=None)
def _long():
    """tests/test_gpu_stage_ref.py::_long_edge with n = 300: point 0 seen by all
    140 cameras (segment chunks)."""
    from bundleadjustmentmatlab_amd.scene import make_config, project
    sc = make_config("cfg2", m=140, n=300, seed=5)
    allc = np.arange(sc.m)
    extra, z = project(sc.K, sc.w, sc.T, sc.X, allc, np.zeros(sc.m, dtype=int))
    assert np.all(z > 0)
    keep = sc.obs_pt != 0
    pt = np.r_[np.zeros(sc.m, int), sc.obs_pt[keep]].astype(np.int32)
    cam = np.r_[allc, sc.obs_cam[keep]].astype(np.int32)
    ox = np.r_[np.asarray(extra).reshape(sc.m, 2), sc.obs_x[keep]]
    order = np.lexsort((cam, pt))
    return sc, pt[order], cam[order], np.ascontiguousarray(ox[order])


@functools.lru_cache(maxsize=None)
def _ladybug():
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("ladybug", m=120, n=12000, seed=3)
    return sc, sc.obs_pt, sc.obs_cam, sc.obs_x


LADDER_TOP = {7: 257, 10: 273, 12: 280}     # as tests/test_gpu_track_lengths.py


def _scene(name, na):
    if name == "ladder":    # tests/track_scenes.py: up to three full segments per track
        import track_scenes as ts
        return ts.ladder(na, LADDER_TOP[na])
    return _long() if name == "long" else _ladybug() if name == "ladybug" else _banded(na)


def _problem(sc, na):
    """(K, a, b, constructor keywords) of the scene's start point."""
    if na == 12:
        from bundleadjustmentmatlab_amd.scene import projective_from
        Pp, Xp = projective_from(sc)
        return (None, np.asfortranarray(Pp.reshape(12, sc.m, order="F")),
                np.asfortranarray(Xp[0:3]), dict(model="projective", m=sc.m))
    a = np.zeros((na, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if na == 7:
        a[6] = sc.K[0]
    elif na == 10:
        a[6:10] = sc.K
    return sc.K, a, np.asfortranarray(sc.X0[:3]), {}


def _make(gpu, K, pt, cam, ox, n, na, fused=True, **kw):
    old = os.environ.pop("VLGBA_FUSED", None)
    if not fused:
        os.environ["VLGBA_FUSED"] = "0"
    try:
        return gpu.BundleAdjuster(K, pt, cam, ox, n, na, **kw)
    finally:
        os.environ.pop("VLGBA_FUSED", None)
        if old is not None:
            os.environ["VLGBA_FUSED"] = old


def _solve(ba, a, b):
    ba.set_params(a, b)
    err, st = ba.run()
    a1, b1 = ba.get_params()
    return (err.copy(), a1.copy(), b1.copy(),
            (st.iterations, st.accepted, st.num_error, st.lambda_, st.pinv_passes,
             st.spin_retries, st.nd_retries))


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


# ---------------------------------------------------------------------------
# 1. bit identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name,na", [("banded", 6), ("banded", 7), ("banded", 10),
                                     ("banded", 12), ("long", 6)])
def test_huber_1e150_run_is_bit_identical_to_no_loss(gpu, name, na, fused):
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    args = (K, pt, cam, ox, sc.n, na)
    with _make(gpu, *args, fused=fused, **kw) as ba:
        plain = _solve(ba, a, b)
        plan = ba.plan_info()
    assert plan["ordered"] == 0 and (name != "long" or plan["long_points"] == 1), plan
    assert plain[3][1] >= 2, plain[3]          # accepted steps: the update kernels ran
    with _make(gpu, *args, fused=fused, loss="huber", loss_scale=1e150, **kw) as ba:
        assert ba.get_loss() == ("huber", 1e150)
        huge = _solve(ba, a, b)
        ba.set_loss("cauchy", SCALE)           # a run with weights that do bite ...
        cauchy = _solve(ba, a, b)
        ba.set_loss("none")                    # ... and back
        assert ba.get_loss() == ("none", 0.0)
        back = _solve(ba, a, b)
    print(f"ROBUST identity {name} num_a {na} fused {fused}: {plain[3][0]} passes, error_ "
          f"{plain[0][0]:.6g} -> {plain[0][-1]:.6g}; cauchy {cauchy[0][0]:.6g} -> "
          f"{cauchy[0][-1]:.6g}")
    assert _same(huge, plain), (huge[0], plain[0], huge[3], plain[3])
    assert not np.array_equal(cauchy[0], plain[0])
    assert _same(back, plain), (back[0], plain[0], back[3], plain[3])


# ---------------------------------------------------------------------------
# 2. stage check
# ---------------------------------------------------------------------------
STAGE = [(name, na, kind, {}) for kind in ("huber", "cauchy")
         for name, na in (("banded", 6), ("banded", 7), ("banded", 10), ("banded", 12),
                          ("long", 6))]
STAGE += [("banded", 6, "huber", dict(pivot="first2")),
          ("banded", 6, "cauchy", dict(fix_structure=True))]
# the _loss segment chunks of the other camera models
STAGE += [("ladder", na, "huber", {}) for na in (7, 10, 12)]


def _dense(sc, pt, cam, ox):
    X = np.zeros((2, sc.n, sc.m), order="F")
    X[0, pt, cam], X[1, pt, cam] = ox[:, 0], ox[:, 1]
    vis = np.zeros((sc.n, sc.m), order="F")
    vis[pt, cam] = 1.0
    return X, vis


@pytest.mark.parametrize("name,na,kind,opt", STAGE,
                         ids=[f"{n}{a}-{k}" + "".join("-" + o for o in sorted(q))
                              for n, a, k, q in STAGE])
def test_weighted_linearisation_within_the_reference_bounds(gpu, oracle, poracle, name, na,
                                                            kind, opt):
    sc, pt, cam, ox = _scene(name, na)
    ox, planted = rr.plant_outliers(ox, seed=13)
    K, a, b, kw = _problem(sc, na)
    kw = dict(kw, **opt)
    pivot = None
    if kw.get("pivot") == "first2":
        pivot = kw["pivot"] = np.arange(sc.m) < 2
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, na, loss=kind, loss_scale=SCALE, **kw) as ba:
        ba.set_params(a, b)
        lin = ba.linearization()
        e, w, rho = ba.residuals()
        info = ba.step(relinearize=False, update_lm=False)
        plan = ba.plan_info()
    assert plan["ordered"] == 0 and (name != "long" or plan["long_points"] == 1), plan
    if name == "ladder":    # the planted tracks of at least 91 views: segment chunks
        import track_scenes as ts
        assert plan["long_points"] == ts.is_long(np.bincount(pt)).sum() >= 10, plan
    X, vis = _dense(sc, pt, cam, ox)
    if na == 12:
        ref1 = poracle.mex1(a, b, X, vis)
        stage_e = gpu.mex_bundle_proj_1_XABeUVWeAeB(a, b, X, vis)[3]
    else:
        ref1 = oracle.mex1(K, a, b, X, vis)
        stage_e = gpu.mex_bundle_1_XABeUVWeAeB(K, a, b, X, vis)[3]
    Ao, Bo, eo = rr.per_obs(ref1[1], ref1[2], ref1[3], pt, cam)
    R = rr.weighted(sc.m, sc.n, na, pt, cam, Ao, Bo, eo, kind, SCALE,
                    fix_structure=bool(opt.get("fix_structure")), pivot=pivot)
    fig = {k: rr.ratio(lin[k], R[k], R[k + "_b"]) for k in ("U", "eA", "V", "eB", "W")}
    fig["w"] = rr.ratio(w, R["w"], R["wbound"])
    fig["rho"] = rr.ratio(rho, R["rho"], R["rhobound"])
    fig["cost"] = rr.ratio(info.old_sse, R["cost"], R["costbound"])
    down = float(np.mean(np.asarray(R["w"], dtype=np.float64) < 1))
    print(f"ROBUST stage {name} num_a {na} {kind} {sorted(opt)}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f"; {planted.sum()} planted of {len(pt)}, {down:.3f} of the weights below 1")
    assert np.array_equal(e, stage_e[:, pt, cam].T)
    assert down > 0.02
    assert all(v <= 1.0 for v in fig.values()), fig
    if pivot is not None:
        assert np.all(lin["U"][:, :, pivot] == 0) and np.all(lin["eA"][:, pivot] == 0)
        assert np.all(lin["W"][:, :, pivot[cam]] == 0) and np.any(lin["W"] != 0)
    if opt.get("fix_structure"):
        assert all(np.all(lin[k] == 0) for k in ("V", "eB", "W")) and np.any(lin["U"] != 0)


def test_residuals_without_a_loss(gpu):
    sc, pt, cam, ox = _banded(6)
    K, a, b, kw = _problem(sc, 6)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6) as ba:
        ba.set_params(a, b)
        e, w, rho = ba.residuals()
        info = ba.step(relinearize=True, update_lm=False)
        e2 = ba.residuals()[0]
    assert np.all(w == 1.0) and np.array_equal(rho, e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    assert abs(rho.sum() - info.old_sse) <= 2 * len(rho) * 2.0 ** -53 * info.old_sse
    assert np.array_equal(e, e2)               # an unapplied pass moves nothing


# ---------------------------------------------------------------------------
# 3. fused against VLGBA_FUSED=0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,na,kind", [("banded", 6, "huber"), ("banded", 10, "cauchy"),
                                          ("long", 6, "cauchy")])
def test_fused_equals_unfused_with_a_loss(gpu, name, na, kind):
    """What tests/test_gpu_fused.py shows without a loss, at its bars: from the
    same start the applied step (da, db, the new a and b) and the linearisation
    at the new point are bit-identical, the old cost too (one linearisation);
    the new cost and dp'(lambda dp + g) agree to summation order (1e-13, 1e-12:
    the fused form sums the new cost from the linearisation's two lanes per
    observation, the separate kernel from one).  A whole run() is therefore not
    bit-identical between the two forms, with or without a loss (measured
    without one: banded num_a 10 and the long-track scene part in the last bit
    of lambda after the first accepted step), so the step is what is compared."""
    sc, pt, cam, ox = _scene(name, na)
    ox, _ = rr.plant_outliers(ox, seed=13)
    K, a, b, kw = _problem(sc, na)
    res = {}
    for fused in (True, False):
        with _make(gpu, K, pt, cam, ox, sc.n, na, fused=fused, loss=kind, loss_scale=SCALE,
                   **kw) as ba:
            ba.set_params(a, b)
            i1 = ba.step(relinearize=False, update_lm=True)
            da, db = ba.last_step()
            res[fused] = (i1, da.copy(), db.copy(), ba.get_params(), ba.linearization(),
                          ba.residuals())
    (fi, ui), f, u = (res[True][0], res[False][0]), res[True], res[False]
    print(f"ROBUST fused {name} num_a {na} {kind}: cost {fi.old_sse:.10g} -> {fi.new_sse:.10g}, "
          f"new cost rel diff {abs(fi.new_sse - ui.new_sse) / ui.new_sse:.2e}, dpg rel diff "
          f"{abs(fi.dpg - ui.dpg) / abs(ui.dpg):.2e}")
    assert fi.accepted == 1 and ui.accepted == 1
    assert fi.old_sse == ui.old_sse
    assert abs(fi.new_sse - ui.new_sse) <= 1e-13 * ui.new_sse, (fi.new_sse, ui.new_sse)
    assert abs(fi.dpg - ui.dpg) <= 1e-12 * abs(ui.dpg), (fi.dpg, ui.dpg)
    assert np.array_equal(f[1], u[1]) and np.array_equal(f[2], u[2])                 # da, db
    assert np.array_equal(f[3][0], u[3][0]) and np.array_equal(f[3][1], u[3][1])     # a, b new
    for nm in ("W", "V", "eB", "U", "eA"):
        assert np.array_equal(f[4][nm], u[4][nm]), (name, nm)
    for q in range(3):
        assert np.array_equal(f[5][q], u[5][q]), q                                 # e, w, rho


# ---------------------------------------------------------------------------
# 4. solvers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded", "ladybug"])
def test_robust_run_on_each_solver(gpu, name):
    sc, pt, cam, ox = _scene(name, 6)
    ox, _ = rr.plant_outliers(ox, seed=13)
    K, a, b, kw = _problem(sc, 6)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, loss="cauchy", loss_scale=SCALE) as ba:
        err, _, _, st = _solve(ba, a, b)
        plan = ba.plan_info()
    print(f"ROBUST solver {name}: cr_levels {plan['cr_levels']} nd_arcs {plan['nd_arcs']} "
          f"error_ {err[0]:.6g} -> {err[-1]:.6g} in {st[0]} passes")
    assert (plan["cr_levels"] > 0) == (name == "banded"), plan
    assert st[4] == 0 and st[1] >= 2 and np.all(np.isfinite(err)) and err[-1] < err[0]
    assert np.all(np.diff(err) < 0)


def test_robust_pinv_pass_lowers_the_cost(gpu):
    sc, pt, cam, ox = _banded(6)
    ox, _ = rr.plant_outliers(ox, seed=13)
    K, a, b, kw = _problem(sc, 6)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, loss="huber", loss_scale=SCALE) as ba:
        ba.set_params(a, b)
        ba.force_status(4, 1)
        info = ba.step(relinearize=True, update_lm=True)
    print(f"ROBUST pinv pass: cost {info.old_sse:.8g} -> {info.new_sse:.8g}")
    assert info.pinv == 1 and info.accepted == 1 and info.new_sse < info.old_sse


# ---------------------------------------------------------------------------
# 5. converged cost, 6. end to end
# ---------------------------------------------------------------------------
def test_converged_robust_cost_survives_the_reference_restart(gpu, oracle):
    sc, ox, _ = rr.e2e_scene()
    K, a, b, kw = _problem(sc, 6)
    c = rr.E2E["scale"]
    with gpu.BundleAdjuster(K, sc.obs_pt, sc.obs_cam, ox, sc.n, 6, loss="cauchy", loss_scale=c,
                            **STOP) as ba:
        err, a1, b1, st = _solve(ba, a, b)
        rho = ba.residuals()[2]
    X, vis = _dense(sc, sc.obs_pt, sc.obs_cam, ox)
    N = float(len(ox))
    # one cost function: the reference's cost at the GPU's parameters
    e_at = oracle.mex1(K, a1, b1, X, vis)[3][:, sc.obs_pt, sc.obs_cam].T
    c_at = rr.cost_of(e_at, "cauchy", c) / N
    _, _, e_r = rr.robust_lm(K, a1, b1, X, vis, "cauchy", c, **STOP)
    final = e_r[-1] if len(e_r) else c_at      # every step rejected: error_ stays empty
    drop = (c_at - final) / c_at
    print(f"ROBUST converged: GPU {err[0]:.8g} -> {err[-1]:.10g} in {st[0]} passes; reference "
          f"cost there {c_at:.10g}; robust_lm from there {final:.10g} (drop {drop:.2e})")
    assert abs(c_at - err[-1]) <= 1e-12 * c_at
    assert abs(rho.sum() / N - err[-1]) <= 1e-12 * err[-1]
    assert -1e-12 <= drop <= 1e-6, drop


def test_end_to_end_outliers(gpu):
    sc, ox, planted = rr.e2e_scene()
    K, a, b, kw = _problem(sc, 6)
    res = {}
    for kind in ("none", "cauchy"):
        with gpu.BundleAdjuster(K, sc.obs_pt, sc.obs_cam, ox, sc.n, 6, loss=kind,
                                loss_scale=rr.E2E["scale"], **rr.E2E["stop"]) as ba:
            err = _solve(ba, a, b)[0]
            assert len(err) >= 2 and err[-1] < err[0]
            res[kind] = ba.residuals()
    fig = rr.e2e_figures(res["none"][0], res["cauchy"][0], res["cauchy"][1], planted)
    print("ROBUST end to end: inlier RMS plain %.4g cauchy %.4g, largest outlier w %.3g, "
          "inliers with w > 0.5: %.4f" % fig)
    rr.e2e_check(fig)


# ---------------------------------------------------------------------------
# 7. arguments
# ---------------------------------------------------------------------------
def test_arguments(gpu):
    sc, pt, cam, ox = _banded(6)
    K, a, b, kw = _problem(sc, 6)
    L = gpu.lib()
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, pivot=np.arange(sc.m) < 2) as ba:
        ba.set_params(a, b)
        for kind in (-1, 3, 99):
            assert L.vlgba_set_loss(ba._h, kind, 1.0) == -1001
        for kind in (1, 2):
            for scale in (0.0, -1.0, float("nan"), float("inf")):
                assert L.vlgba_set_loss(ba._h, kind, scale) == -1001
        assert ba.get_loss() == ("none", 0.0)              # a refused call changes nothing
        assert L.vlgba_set_loss(ba._h, 0, float("nan")) == 0   # no scale without a loss
        with pytest.raises(ValueError):
            ba.set_loss("tukey", 1.0)
        ba.set_loss("cauchy", 2.5)
        assert ba.get_loss() == ("cauchy", 2.5)
        with pytest.raises(gpu.VlgbaError, match="-1001"):
            ba.covariance(scale=True)
        cov = ba.covariance(scale=False)
        rho = ba.residuals()[2]
        assert abs(cov["sse"] - rho.sum()) <= 1e-12 * cov["sse"]   # info[0]: the robust cost
        assert np.all(np.isfinite(cov["cam"])) and np.all(cov["cam"][:, :, :2] == 0)
    for mode in (dict(parity=True), dict(ordered=True)):
        with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, **mode) as ba:
            assert L.vlgba_set_loss(ba._h, 1, 3.0) == -1001
            assert L.vlgba_set_loss(ba._h, 0, 0.0) == -1001
        with pytest.raises(ValueError):
            gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, loss="huber", loss_scale=3.0, **mode)


def test_drivers_take_the_loss(gpu):
    sc, ox, planted = rr.e2e_scene()
    x = np.zeros((3, sc.n, sc.m), order="F")
    x[0, sc.obs_pt, sc.obs_cam], x[1, sc.obs_pt, sc.obs_cam] = ox[:, 0], ox[:, 1]
    x[2, sc.obs_pt, sc.obs_cam] = 1.0
    vis = sc.dense()[1]
    opts = ("visibility", vis, "fix_calibration")
    plain = gpu.bundle_euclid(sc.K, sc.T0, sc.w0, sc.X0, x, *opts)[4]
    dense = gpu.bundle_euclid(sc.K, sc.T0, sc.w0, sc.X0, x, *opts, loss="cauchy",
                              loss_scale=SCALE)[4]
    obs = gpu.bundle_euclid_obs(sc.K, sc.T0, sc.w0, sc.X0, sc.obs_pt, sc.obs_cam, ox,
                                "fix_calibration", loss="cauchy", loss_scale=SCALE)[4]
    assert np.array_equal(dense, obs) and dense[0] < plain[0]   # rho(s) < s for s > 0
    with pytest.raises(ValueError):
        gpu.bundle_euclid(sc.K, sc.T0, sc.w0, sc.X0, x, *opts, loss="huber", loss_scale=SCALE,
                          parity=True)


# ---------------------------------------------------------------------------
# 8. two ranks
# ---------------------------------------------------------------------------
def test_two_rank_threads_match_one_rank(gpu):
    """Two rank threads on one GPU (dist.HostGroup, as tests/test_gpu_dist.py)
    against the one-rank passes, at that file's bars for the same comparison
    without a loss: identical decisions, the first old cost 1e-11, the first
    new cost 1e-7, every cost 1e-4 relative."""
    import threading
    from bundleadjustmentmatlab_amd.dist import HostGroup
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=40, n=5000, seed=21)
    ox, _ = rr.plant_outliers(sc.obs_x, seed=13)
    K, a, b, kw = _problem(sc, 6)
    args = (K, sc.obs_pt, sc.obs_cam, ox, sc.n, 6)
    loss = dict(loss="cauchy", loss_scale=SCALE)

    def passes(ba):
        ba.set_params(a, b)
        infos = [ba.step(relinearize=True, update_lm=True) for _ in range(3)]
        return ([i.old_sse for i in infos], [i.new_sse for i in infos],
                [i.accepted for i in infos], ba.plan_info())

    with gpu.BundleAdjuster(*args, **loss) as ba:
        one = passes(ba)
    world = 2
    grp = HostGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            with gpu.BundleAdjuster(*args, rank=r, world_size=world,
                                    allreduce=grp.allreduce_fn(r), **loss) as ba:
                out[r] = passes(ba)
        except Exception as e:   # noqa: BLE001 -- re-raised below
            errs.append(e)
            grp._bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert sum(o[3]["points"] for o in out) == sc.n and all(not o[3]["ordered"] for o in out)
    assert out[0][:3] == out[1][:3]                      # replicated decisions and costs
    old, new, acc, _ = out[0]
    print(f"ROBUST two ranks: old {old} new {new} | one rank old {one[0]} new {one[1]}")
    assert acc == one[2] and sum(acc) >= 2
    assert abs(old[0] - one[0][0]) <= 1e-11 * one[0][0]
    assert abs(new[0] - one[1][0]) <= 1e-7 * one[1][0]
    assert np.allclose(old, one[0], rtol=1e-4, atol=0)
    assert np.allclose(new, one[1], rtol=1e-4, atol=0)
