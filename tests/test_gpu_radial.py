"""The radial-distortion camera (num_a = 9: a = [w; T; f; k1; k2], include/vlgba.h,
DESIGN.md sec. 5) on the fast path against tests/radial_ref.py, which
tests/test_radial_ref.py proves on the CPU.

The scenes are those of tests/test_gpu_robust.py (banded with 34 cameras: cyclic
reduction on 27-row tiles, the last tile one camera; "long": one point seen by
140 cameras; ladybug-120: nested dissection / envelope) and a
tests/track_scenes.py scene with planted tracks of 7 and 8 views (BA_MF_CMAX(9)
| + 1: MFMA and per-term Schur groups in one plan), their observations generated
anew in numpy under the ground-truth distortion k1 = -0.15, k2 = 0.03 plus
0.5 px noise.  The start has the scenes' perturbed poses and points and
coefficients 10 % / 20 % off, so every term of the Jacobian is alive.

1. linearization()'s U, eA, V, eB, W within radial_ref's propagated bounds
   (ratio <= 1), pivot cameras and fix_structure with their exact zeros.
2. residuals(), step().old_sse and step().new_sse -- the latter at the returned
   a_new, b_new -- within the reference's own bounds, with the fused update and
   with VLGBA_FUSED=0 (k_point_update_chunk's own projection).
3. One pass: schur_kernel="terms" and solver="dense" against auto at
   tests/test_gpu_nd.py's bars (1e-9 on da, db); the folded camera update on and
   off, bit-identical.  (GPU against GPU.  The Schur complement, every solver
   and the update at num_a = 9 are held to the references entry by entry in
   tests/test_gpu_stage_ref.py's radial9-* and *-na9 cases, the chunk kinds of
   k_schur_mfma in tests/test_gpu_schur_head_na.py, and the long tracks and
   k_point_cov's LDS edge in tests/test_gpu_track_lengths.py's ladder-9,
   ladder-9-over and shared-257-na9.)
4. A whole LM run from k = 0: the reference LM started at the GPU's answer
   lowers the cost by at most 1e-6 relative (the project's restart bar).
5. Huber at 1e150 is bit-identical to no loss; one Huber pass with planted
   outliers matches the weighted reference; covariance() at the bars of
   tests/test_gpu_covariance.py with the reference's linearisation.
6. Arguments: analytic only, no ordered / parity mode, no resect / stage entries.
7. Two rank threads against one rank, at tests/test_gpu_dist.py's bars.

Every test prints its figures before it asserts (lines starting RADIAL, pytest -s;
profiles/radial/gpu_tests.log keeps a run).  Measured on an MI355X; no bar was
widened.  Largest |diff| / bound of the stage check over its cases: U 0.067, eA
0.053, V 0.064, eB 0.049, W 0.15 (all on the planted tracks; banded: 0.017,
0.015, 0.039, 0.032, 0.061).  Residuals 0.23 of their bound (about 4e-12 px),
old_sse 0.0026, new_sse 0.00070 of theirs (1e-8 .. 5e-8 on costs of 2e3 .. 9e3),
fused and unfused alike; the pinhole cost at the same start is 30 times the
model's.  Solvers on one pass: da within 1.7e-13, db 1.9e-14 (bar 1e-9).  Huber
pass: w 0.21, rho 0.20, cost 1.3e-4, new cost 3.2e-5 of their bounds.  LM run
from k = 0: error_ 475.88 -> 0.346768736163 in 32 passes; the reference LM from
there lowers it by 1.4e-13 relative (bar 1e-6); recovered k1 -0.165 .. -0.145
(truth -0.15), k2 0.024 .. 0.059 (truth 0.03), the reference's within 6e-8.
Covariance, cond(S0) 1.6e11: camera blocks 5.6e-10 against the fp64 floor
1.5e-9, points 0.90 of their bound, end to end 6.6e-10 (floor 2.0e-9).
"""
import ctypes
import functools

import numpy as np
import pytest

import radial_ref as ra
import robust_ref as rr
import test_gpu_robust as scenes
from test_gpu_jacobian import _make as _make_env
from test_gpu_robust import _same, _solve

pytestmark = pytest.mark.gpu

NA = 9
NOISE = 0.5
K_START = (0.9, 1.2)        # the start's coefficients as multiples of the truth
PLANT_M, PLANT_N = 40, 300


@functools.lru_cache(maxsize=None)
def _planted():
    """Six windows of 7 consecutive cameras and six of 8, on a ladybug base whose
    own tracks have up to 30 views (both Schur kinds either way)."""
    import track_scenes as ts
    tracks = [list(range(s, s + k)) for k in (7, 8) for s in (0, 5, 11, 18, 26, 32)]
    return ts.planted(PLANT_M, PLANT_N, tracks, seed=11)


@functools.lru_cache(maxsize=None)
def _rscene(name):
    """The scene under the lens: dict K, a0 (9, m), b0, a_true, pt, cam, obs_x, m, n."""
    if name == "planted":
        sc, pt, cam, _ = _planted()
    else:
        sc, pt, cam, _ = scenes._scene(name, 10 if name == "banded" else 6)
    kt = np.tile(np.array(ra.K_TRUE)[:, None], (1, sc.m))
    a_true = ra.pack(sc.K, sc.w, sc.T, kt)
    ox = ra.observe(sc.K, a_true, sc.X, pt, cam, NOISE, 77)
    a0 = ra.pack(sc.K, sc.w0, sc.T0, kt * np.array(K_START)[:, None])
    return dict(K=sc.K, a0=a0, b0=np.asfortranarray(sc.X0[:3]), a_true=a_true, pt=pt, cam=cam,
                obs_x=ox, m=sc.m, n=sc.n)


def _ba(gpu, s, fused=True, env=None, obs_x=None, **kw):
    ox = s["obs_x"] if obs_x is None else obs_x
    if env is not None:
        return _make_env(gpu, s["K"], s["pt"], s["cam"], ox, s["n"], NA, env=env, **kw)
    return scenes._make(gpu, s["K"], s["pt"], s["cam"], ox, s["n"], NA, fused=fused, **kw)


def _check_plan(name, plan, pt):
    assert plan["ordered"] == 0 and plan["num_a"] == NA, plan
    if name == "banded":      # 34 cameras: 11 tiles of three and one of one
        assert plan["cr_levels"] > 0 and plan["cr_rows"] == 27 and plan["cameras"] % 3 == 1, plan
    if name == "long":
        assert plan["long_points"] == 1, plan
    if name == "planted":
        k = np.bincount(pt)[PLANT_N:]
        assert sorted(set(k)) == [7, 8] and 0 < plan["mfma_groups"] < plan["groups"], plan
    if name == "ladybug":
        assert plan["cr_levels"] == 0, plan


# ---------------------------------------------------------------------------
# 1. the linearisation
# ---------------------------------------------------------------------------
STAGE = [("banded", {}), ("long", {}), ("planted", {}), ("banded", dict(pivot="first2")),
         ("banded", dict(fix_structure=True))]


@pytest.mark.parametrize("name,opt", STAGE,
                         ids=[n + "".join("-" + o for o in sorted(q)) for n, q in STAGE])
def test_linearisation_within_the_reference_bounds(gpu, name, opt):
    """Measured, largest |diff| / bound over all cases: U 0.067, eA 0.053, V 0.064,
    eB 0.049, W 0.15 (the planted tracks; the 140-view track: 0.030, 0.023, 0.026,
    0.017, 0.062).  The W bounds are 5e-10 .. 6e-8 of |W| at most."""
    s = _rscene(name)
    kw = dict(opt)
    pivot = None
    if kw.get("pivot") == "first2":
        pivot = kw["pivot"] = np.arange(s["m"]) < 2
    with _ba(gpu, s, **kw) as ba:
        assert ba.get_jacobian() == "analytic"
        ba.set_params(s["a0"], s["b0"])
        lin = ba.linearization()
        e = ba.residuals()[0]
        plan = ba.plan_info()
    _check_plan(name, plan, s["pt"])
    R = ra.linearization(s["K"], s["a0"], s["b0"], s["pt"], s["cam"], e, s["m"], s["n"],
                         fix_structure=bool(opt.get("fix_structure")), pivot=pivot)
    fig = {k: rr.ratio(lin[k], R[k], R[k + "_b"]) for k in ("U", "eA", "V", "eB", "W")}
    Wref = np.asarray(R["W"], dtype=np.float64)
    nz = Wref != 0
    rel = float((np.asarray(R["W_b"], dtype=np.float64)[nz] / np.abs(Wref[nz])).max()) \
        if nz.any() else float("nan")
    print(f"RADIAL stage {name} {sorted(opt)}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f"; {len(s['pt'])} observations, largest W bound / |W| {rel:.2e}")
    assert all(v <= 1.0 for v in fig.values()), fig
    if opt.get("fix_structure"):
        assert all(np.all(lin[k] == 0) for k in ("V", "eB", "W")) and np.any(lin["U"] != 0)
    else:
        assert np.all(np.abs(lin["W"][6:9]).max(axis=(1, 2)) > 0)    # f, k1, k2 rows alive
    if pivot is not None:
        assert np.all(lin["U"][:, :, pivot] == 0) and np.all(lin["eA"][:, pivot] == 0)
        assert np.all(lin["W"][:, :, pivot[s["cam"]]] == 0) and np.any(lin["W"] != 0)


# ---------------------------------------------------------------------------
# 2. residuals and the costs of a pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", ["banded", "long", "planted"])
def test_residuals_and_costs_within_the_reference_bounds(gpu, name, fused):
    """The bars are the reference's own bounds (a few 1e-13 px per residual).  A
    pinhole projection left in an update kernel misses new_sse by the lens's
    whole effect."""
    s = _rscene(name)
    K, pt, cam, ox = s["K"], s["pt"], s["cam"], s["obs_x"]
    with _ba(gpu, s, fused=fused) as ba:
        ba.set_params(s["a0"], s["b0"])
        e = ba.residuals()[0]
        info = ba.step(relinearize=True, update_lm=True)
        da, db = ba.last_step()
        a1, b1 = ba.get_params()
        info2 = ba.step(relinearize=True, update_lm=False)
    eref, eb = ra.residuals(K, s["a0"], s["b0"], pt, cam, ox)
    c0, c0b = ra.cost(K, s["a0"], s["b0"], pt, cam, ox)
    c1, c1b = ra.cost(K, a1, b1, pt, cam, ox)
    pin = s["a0"].copy()
    pin[7:9] = 0
    fig = dict(e=rr.ratio(e, eref, eb), old_sse=rr.ratio(info.old_sse, c0, c0b),
               new_sse=rr.ratio(info.new_sse, c1, c1b), next_old_sse=rr.ratio(info2.old_sse, c1, c1b))
    print(f"RADIAL costs {name} fused {fused}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f"; cost {info.old_sse:.10g} -> {info.new_sse:.10g} (bounds {float(c0b):.2e}, "
          f"{float(c1b):.2e}; the pinhole cost at the start: "
          f"{float(ra.cost(K, pin, s['b0'], pt, cam, ox)[0]):.6g})")
    assert info.accepted == 1 and info.new_sse < info.old_sse
    assert np.array_equal(a1, s["a0"] + da) and np.array_equal(b1, s["b0"] + db)
    assert np.all(da[6:9] != 0)
    assert all(v <= 1.0 for v in fig.values()), fig


def test_semantics_do_not_change_the_step(gpu):
    """All nine rows of da enter the back substitution under either semantics."""
    s = _rscene("banded")
    res = []
    for sem in ("mex", "nomex"):
        with _ba(gpu, s, semantics=sem) as ba:
            ba.set_params(s["a0"], s["b0"])
            info = ba.step(relinearize=True, update_lm=False)
            res.append((info.new_sse, info.dpg) + ba.last_step())
    assert res[0][:2] == res[1][:2]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


# ---------------------------------------------------------------------------
# 3. the solvers on one pass
# ---------------------------------------------------------------------------
def _pass(gpu, s, env=None, **kw):
    with _ba(gpu, s, env=env, **kw) as ba:
        ba.set_params(s["a0"], s["b0"])
        info = ba.step(relinearize=True, update_lm=False)
        da, db = ba.last_step()
        return info, da.copy(), db.copy(), ba.plan_info()


@pytest.mark.parametrize("name,kw", [("banded", dict(schur_kernel="terms")),
                                     ("planted", dict(schur_kernel="terms")),
                                     ("banded", dict(solver="dense")),
                                     ("ladybug", dict(solver="dense")),
                                     ("ladybug", dict(solver="nd"))],
                         ids=["banded-terms", "planted-terms", "banded-dense", "ladybug-dense",
                              "ladybug-nd"])
def test_solvers_agree_on_one_pass(gpu, name, kw):
    s = _rscene(name)
    i0, da0, db0, p0 = _pass(gpu, s)
    i1, da1, db1, p1 = _pass(gpu, s, **kw)
    _check_plan(name, p0, s["pt"])
    if "schur_kernel" in kw:
        assert p0["mfma_groups"] > 0 and p1["mfma_groups"] == 0, (p0, p1)
    elif kw["solver"] == "nd":
        assert p1["cr_levels"] == 0 and p1["nd_arcs"] >= 2, p1
    else:
        assert p1["cr_levels"] == 0 and p1["nd_arcs"] == 0, p1
    fa = np.max(np.abs(da1 - da0)) / np.max(np.abs(da0))
    fb = np.max(np.abs(db1 - db0)) / np.max(np.abs(db0))
    print(f"RADIAL solvers {name} {kw}: da {fa:.2e} db {fb:.2e} new_sse "
          f"{abs(i1.new_sse - i0.new_sse) / i0.new_sse:.2e} (cr_levels {p0['cr_levels']} nd_arcs "
          f"{p0['nd_arcs']} mfma groups {p0['mfma_groups']} of {p0['groups']})")
    assert i0.chol_failed == 0 and i1.chol_failed == 0 and i0.pinv == 0 and i1.pinv == 0
    # (another chunk plan sums the cost in another order: the bound of an N-term sum)
    assert abs(i0.old_sse - i1.old_sse) <= 2 * len(s["pt"]) * 2.0 ** -53 * i0.old_sse
    assert fa <= 1e-9 and fb <= 1e-9, (fa, fb)
    assert abs(i1.new_sse - i0.new_sse) <= 1e-9 * i0.new_sse


def test_cyclic_reduction_with_and_without_the_folded_camera_update(gpu):
    s = _rscene("banded")
    res = {}
    for fold in (True, False):
        with _ba(gpu, s, env={"VLGBA_CAMUPD_FOLD": None if fold else "0"}) as ba:
            res[fold] = _solve(ba, s["a0"], s["b0"])
            plan = ba.plan_info()
        assert plan["cr_levels"] > 0 and plan["cr_rows"] == 27, plan
        assert plan["camupd_fold"] == int(fold), plan
    err, st = res[True][0], res[True][3]
    print(f"RADIAL cyclic reduction: cr_levels {plan['cr_levels']} tiles of {plan['cr_rows']} "
          f"rows, error_ {err[0]:.6g} -> {err[-1]:.10g} in {st[0]} passes")
    assert st[4] == 0 and st[1] >= 2 and np.all(np.diff(err) < 0)
    assert _same(res[True], res[False])


# ---------------------------------------------------------------------------
# 4. a whole LM run
# ---------------------------------------------------------------------------
def test_lm_run_from_zero_coefficients_survives_the_reference_restart(gpu):
    """Measured: 32 passes, all accepted, error_ 475.88188 -> 0.346768736163; the
    reference LM from there: drop 1.35e-13 relative; largest |k GPU - k
    reference| 6.0e-8."""
    from bundleadjustmentmatlab_amd import bundle_euclid_obs
    s = ra.e2e_scene()
    K, pt, cam, ox, free = s["K"], s["pt"], s["cam"], s["obs_x"], ~s["pivot"]
    assert np.all(s["a0"][7:9][:, free] == 0)
    with gpu.BundleAdjuster(K, pt, cam, ox, s["n"], NA, pivot=s["pivot"], **ra.E2E["stop"]) as ba:
        err, a1, b1, st = _solve(ba, s["a0"], s["b0"])
    N = float(len(pt))
    c_at = float(ra.cost(K, a1, b1, pt, cam, ox)[0]) / N
    a_r, _, e_r = ra.radial_lm(K, a1, b1, pt, cam, ox, pivot=s["pivot"], **ra.E2E["stop"])
    final = e_r[-1] if len(e_r) else c_at
    drop = (c_at - final) / c_at
    rng = lambda x: f"{x[free].min():.5f} .. {x[free].max():.5f}"
    print(f"RADIAL lm: GPU error_ {err[0]:.8g} -> {err[-1]:.12g} in {st[0]} passes ({st[1]} "
          f"accepted); reference cost there {c_at:.12g}; radial_lm from there {final:.12g} "
          f"(drop {drop:.2e})")
    print(f"RADIAL lm coefficients: k1 GPU {rng(a1[7])} reference {rng(a_r[7])} truth "
          f"{ra.K_TRUE[0]}; k2 GPU {rng(a1[8])} reference {rng(a_r[8])} truth {ra.K_TRUE[1]}; "
          f"largest |k GPU - k reference| {np.abs(a1[7:9] - a_r[7:9]).max():.2e}")
    assert st[4] == 0 and np.all(np.diff(err) < 0)
    assert err[-1] < 1.0 < err[0]            # the noise floor of an exact fit is 0.5 px^2
    assert np.array_equal(a1[:, s["pivot"]], s["a0"][:, s["pivot"]])
    assert abs(c_at - err[-1]) <= 1e-12 * c_at
    assert -1e-12 <= drop <= 1e-6, drop
    # the driver: the same run through bundle_euclid_obs(radial=), bit for bit
    Xe = np.vstack([s["b0"], np.ones((1, s["n"]))])
    out = bundle_euclid_obs(K, s["a0"][3:6], s["a0"][0:3], Xe, pt, cam, ox, "fix_pivot",
                            s["pivot"], radial=s["a0"][7:9], **ra.E2E["stop"])
    assert len(out) == 6
    assert np.array_equal(out[5], a1[7:9]) and np.array_equal(out[4], err)
    assert np.array_equal(out[0][0], a1[6]) and np.array_equal(out[0][2:4], K[2:4])
    assert np.array_equal(out[1], a1[3:6]) and np.array_equal(out[2], a1[0:3])
    assert np.array_equal(out[3][0:3], b1)


# ---------------------------------------------------------------------------
# 5. with the other features
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("banded", True), ("banded", False), ("long", True)])
def test_huber_1e150_is_bit_identical_to_no_loss(gpu, name, fused):
    s = _rscene(name)
    with _ba(gpu, s, fused=fused) as ba:
        plain = _solve(ba, s["a0"], s["b0"])
    with _ba(gpu, s, fused=fused, loss="huber", loss_scale=1e150) as ba:
        huge = _solve(ba, s["a0"], s["b0"])
        ba.set_loss("cauchy", 3.0)
        cauchy = _solve(ba, s["a0"], s["b0"])
    print(f"RADIAL identity {name} fused {fused}: {plain[3][0]} passes, error_ {plain[0][0]:.6g} "
          f"-> {plain[0][-1]:.6g}; cauchy -> {cauchy[0][-1]:.6g}")
    assert plain[3][1] >= 2
    assert _same(huge, plain), (huge[0], plain[0])
    assert not np.array_equal(cauchy[0], plain[0])


@pytest.mark.parametrize("name", ["banded", "long"])
def test_one_huber_pass_matches_the_weighted_reference(gpu, name):
    s = _rscene(name)
    ox, planted = rr.plant_outliers(s["obs_x"], seed=13)
    K, pt, cam = s["K"], s["pt"], s["cam"]
    with _ba(gpu, s, obs_x=ox, loss="huber", loss_scale=3.0) as ba:
        ba.set_params(s["a0"], s["b0"])
        lin = ba.linearization()
        e, w, rho = ba.residuals()
        info = ba.step(relinearize=False, update_lm=True)
        a1, b1 = ba.get_params()
    eref, eb = ra.residuals(K, s["a0"], s["b0"], pt, cam, ox)
    R = ra.linearization(K, s["a0"], s["b0"], pt, cam, e, s["m"], s["n"], kind="huber", c=3.0)
    fig = {k: rr.ratio(lin[k], R[k], R[k + "_b"]) for k in ("U", "eA", "V", "eB", "W")}
    fig["e"] = rr.ratio(e, eref, eb)
    fig["w"] = rr.ratio(w, R["w"], R["wbound"])
    fig["rho"] = rr.ratio(rho, R["rho"], R["rhobound"])
    fig["cost"] = rr.ratio(info.old_sse, R["cost"], R["costbound"])
    # the new cost: the robust cost of the reference's residuals at the new point, with the
    # bound of its sum and of the residuals under rho (|rho'| <= 1: at most 2 |e| de each)
    e1, e1b = ra.residuals(K, a1, b1, pt, cam, ox)
    s1 = (e1 * e1).sum(1)
    _, rho1, mag1 = rr.loss("huber", 3.0, s1)
    c1b = (2 * np.abs(e1) * e1b).sum() + (len(pt) - 1 + rr.KRHO) * rr.U53 * mag1.sum()
    fig["new_cost"] = rr.ratio(info.new_sse, rho1.sum(), c1b)
    down = float(np.mean(np.asarray(R["w"], dtype=np.float64) < 1))
    print(f"RADIAL huber {name}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f"; {planted.sum()} planted of {len(pt)}, {down:.3f} of the weights below 1; cost "
          f"{info.old_sse:.8g} -> {info.new_sse:.8g}")
    assert down > 0.02 and info.accepted == 1
    assert all(v <= 1.0 for v in fig.values()), fig


def test_covariance(gpu):
    """tests/test_gpu_covariance.py's camera stage, point stage and end-to-end
    check at its bars, its references fed radial_ref's linearisation (rounded to
    fp64); dense and selected methods."""
    import cov_ref as cr
    import test_gpu_covariance as tc
    s = _rscene("banded")
    K, pt, cam, m, n = s["K"], s["pt"], s["cam"], s["m"], s["n"]
    pivot = np.arange(m) < 2
    with _ba(gpu, s, pivot=pivot) as ba:
        ba.set_params(s["a0"], s["b0"])
        e = ba.residuals()[0]
        glin = ba.linearization()
        cov = ba.covariance(scale=False, full=True)
        sel = ba.covariance(scale=False, method="selected", blocks=True)
        plan = ba.plan_info()
    assert plan["cr_levels"] > 0 and plan["cr_rows"] == 27, plan
    R = ra.linearization(K, s["a0"], s["b0"], pt, cam, e, m, n, pivot=pivot)
    lin = {k: np.asfortranarray(np.asarray(R[k], dtype=np.float64))
           for k in ("U", "eA", "V", "eB", "W")}
    assert all(rr.ratio(glin[k], R[k], R[k + "_b"]) <= 1.0 for k in lin)
    r = dict(lin=lin, na=NA, m=m, n=n, pt=pt, cam=cam)
    ref = tc._camera_ref(r, "radial-banded9")
    full, fixed = cov["full"], ref["fixed"]
    fig_full = cr.block_figure(full, ref["want"], NA)
    fig_diag = cr.block_figure(cov["cam"], cr.diag_blocks(ref["want"], NA), NA)
    pref, bound = cr.point_cov(NA, pt, cam, lin["W"], ref["Vi"], full)
    ratio = cr.point_ratio(cov["pts"], pref, bound)
    seen = np.bincount(pt, minlength=n) > 0
    full_a, full_b, _ = cr.normal_inverse(NA, m, n, pt, cam, lin["U"], lin["V"], lin["W"], fixed,
                                          seen)
    b64 = cr.point_cov_fp64(NA, pt, cam, lin["W"], ref["Vi"], ref["inv64"])
    floor_a, floor_b = cr.block_figure(ref["inv64"], full_a, NA), cr.block_figure(b64, full_b, 3)
    fig_a, fig_b = cr.block_figure(full, full_a, NA), cr.block_figure(cov["pts"], full_b, 3)
    # the selected method: its diagonal blocks and co-visible blocks against the same inverse
    sel_diag = cr.block_figure(sel["cam"], cr.diag_blocks(ref["want"], NA), NA)
    want_blk = np.stack([ref["want"][NA * j:NA * j + NA, NA * k:NA * k + NA]
                         for j, k in sel["blk_jk"]])
    sel_blk = float(np.abs(sel["blocks"] - want_blk).max() / np.abs(want_blk).max())
    print(f"RADIAL covariance: fixed rows {int(fixed.sum())} cond(S0) {ref['cond']:.2g}; cameras: "
          f"diagonal blocks GPU {fig_diag:.3g} numpy {ref['floor_diag']:.3g}, all blocks GPU "
          f"{fig_full:.3g} numpy {ref['floor_full']:.3g}; points {ratio:.3g} of the bound; end "
          f"to end cameras {fig_a:.3g} floor {floor_a:.3g}, points {fig_b:.3g} floor "
          f"{floor_b:.3g}; selected: diagonal {sel_diag:.3g}, co-visible blocks {sel_blk:.3g} of "
          f"the largest entry")
    assert np.array_equal(full, full.T) and np.all(np.isfinite(full))
    assert np.all(full[fixed, :] == 0.0) and cov["fixed_rows"] == int(fixed.sum()) == 2 * NA
    assert fig_diag <= 8 * ref["floor_diag"] and fig_full <= 8 * ref["floor_full"]
    assert ratio <= 1.0, ratio
    assert fig_a <= 8 * floor_a and fig_b <= 8 * floor_b
    assert sel_diag <= 8 * ref["floor_diag"]
    assert np.all(np.isfinite(sel["blocks"])) and sel["fixed_rows"] == 2 * NA


# ---------------------------------------------------------------------------
# 6. arguments
# ---------------------------------------------------------------------------
def test_arguments(gpu):
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions, VlgbaResectProblem, VlgbaStats
    s = _rscene("banded")
    L = gpu.lib()
    with _ba(gpu, s) as ba:
        assert ba.get_jacobian() == "analytic"
        assert L.vlgba_set_jacobian(ba._h, 0) == -1001
        with pytest.raises(gpu.VlgbaError, match="-1001"):
            ba.set_jacobian("fd")
        assert ba.get_jacobian() == "analytic"          # a refused call changes nothing
        ba.set_jacobian("analytic")
    with pytest.raises(gpu.VlgbaError, match="-1001"):
        _ba(gpu, s, jacobian="fd")
    for env in ("fd", "analytic"):                      # VLGBA_JACOBIAN has no effect
        with _ba(gpu, s, env={"VLGBA_JACOBIAN": env}) as ba:
            assert ba.get_jacobian() == "analytic"
    for mode in (dict(parity=True), dict(ordered=True)):
        with pytest.raises(gpu.VlgbaError, match="-1001"):
            _ba(gpu, s, **mode)
    # a problem the planner hands to the ordered kernels although ordered == 0 is asked for
    from test_gpu_jacobian import _planner_ordered
    sc, pt, cam, ox = _planner_ordered()
    with pytest.raises(gpu.VlgbaError, match="-1001"):
        gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, NA)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 7) as ba:
        assert ba.plan_info()["ordered"] == 1
    # num_a = 8 stays what tests/test_abi.py pins
    with pytest.raises(gpu.VlgbaError, match="-1002"):
        gpu.BundleAdjuster(s["K"], s["pt"], s["cam"], s["obs_x"], s["n"], 8)
    # resect: one camera, four points
    ptr = np.array([0, 4], dtype=np.int64)
    X = np.ascontiguousarray(np.random.default_rng(0).uniform(-1, 1, (4, 3)) + [0, 0, 5.0])
    x = np.zeros((4, 2))
    a = np.zeros(9)
    a[6] = 500.0
    Kc = np.array([500.0, 500.0, 0.0, 0.0])
    dp = lambda q: q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    pr = VlgbaResectProblem(1, NA, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), dp(X),
                            dp(x), dp(Kc))
    err, nerr = np.zeros(21), np.zeros(1, dtype=np.int32)
    opt, st = VlgbaOptions(), VlgbaStats()
    rc = L.vlgba_resect(ctypes.byref(pr), ctypes.byref(opt), dp(a), dp(err), 21,
                        nerr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(st))
    assert rc == -1002
    # the MEX stage entries
    m, n = 3, 5
    rng = np.random.default_rng(1)
    K3 = np.tile(np.array([[500.0], [500.0], [0.0], [0.0]]), (1, m))
    a9 = np.zeros((NA, m))
    a9[5], a9[6] = 5.0, 500.0
    b = rng.uniform(-1, 1, (3, n))
    Xd, vis = np.zeros((2, n, m)), np.ones((n, m))
    with pytest.raises(gpu.VlgbaError, match="-1002"):
        gpu.mex_bundle_1_XABeUVWeAeB(K3, a9, b, Xd, vis)
    W = rng.standard_normal((NA, 3, n, m))
    with pytest.raises(gpu.VlgbaError, match="-1002"):
        gpu.mex_bundle_2_Se_(W, W, np.zeros((NA, NA, m)), np.zeros((NA, m)), np.zeros((3, n)))
    with pytest.raises(gpu.VlgbaError, match="-1002"):
        gpu.mex_bundle_3_db_new(W, np.zeros((NA * m, 1)), np.zeros((3, n)), np.zeros((3, 3, n)),
                                K3, a9, b, Xd, vis)


def test_two_rank_threads_match_one_rank(gpu):
    """tests/test_gpu_jacobian.py's two-rank comparison (the bars of
    tests/test_gpu_dist.py) at num_a = 9."""
    import threading
    from bundleadjustmentmatlab_amd.dist import HostGroup
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=40, n=5000, seed=21)
    kt = np.tile(np.array(ra.K_TRUE)[:, None], (1, sc.m))
    ox = ra.observe(sc.K, ra.pack(sc.K, sc.w, sc.T, kt), sc.X, sc.obs_pt, sc.obs_cam, NOISE, 78)
    a = ra.pack(sc.K, sc.w0, sc.T0, kt * np.array(K_START)[:, None])
    b = np.asfortranarray(sc.X0[:3])
    args = (sc.K, sc.obs_pt, sc.obs_cam, ox, sc.n, NA)

    def passes(ba):
        assert ba.get_jacobian() == "analytic"
        ba.set_params(a, b)
        infos = [ba.step(relinearize=True, update_lm=True) for _ in range(3)]
        return ([i.old_sse for i in infos], [i.new_sse for i in infos],
                [i.accepted for i in infos], ba.plan_info())

    with gpu.BundleAdjuster(*args) as ba:
        one = passes(ba)
    world = 2
    grp = HostGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            with gpu.BundleAdjuster(*args, rank=r, world_size=world,
                                    allreduce=grp.allreduce_fn(r)) as ba:
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
    assert out[0][:3] == out[1][:3]
    old, new, acc, _ = out[0]
    print(f"RADIAL two ranks: old {old} new {new} | one rank old {one[0]} new {one[1]}")
    assert acc == one[2] and sum(acc) >= 2
    assert abs(old[0] - one[0][0]) <= 1e-11 * one[0][0]
    assert abs(new[0] - one[1][0]) <= 1e-7 * one[1][0]
    assert np.allclose(old, one[0], rtol=1e-4, atol=0)
    assert np.allclose(new, one[1], rtol=1e-4, atol=0)
