"""Analytic Jacobians on the fast path (jacobian="analytic", vlgba_set_jacobian,
DESIGN.md sec. 5) against tests/jac_ref.py, which tests/test_jac_ref.py proves
on the CPU.  The scenes are those of tests/test_gpu_robust.py.

1. Stage: linearization()'s U, eA, V, eB, W within the bounds jac_ref
   propagates from its per-entry Jacobian bounds through the sums' own
   (robust_ref.weighted with w = 1): banded num_a 6 / 7 / 10 / 12, the 140-view
   track, the ladders; pivots and fix_structure keep their exact zeros.  The FD
   linearisation of the same contexts lies outside those bounds for more than
   half of the nonzero W entries.
2. What must not move: residuals() and step().old_sse bit-equal between the two
   modes at equal parameters; set_jacobian("fd") after an analytic run gives a
   fresh FD context's run() bit for bit.
3. Fused against VLGBA_FUSED=0 in analytic mode at the bars of
   tests/test_gpu_fused.py; Huber at scale 1e150 bit-identical to no loss (the
   LOSS x JAC instantiations).
4. Solvers: cyclic reduction with the camera update inside k_cr32_fused<true> and
   with VLGBA_CAMUPD_FOLD=0 (k_camera_update_jac), bit-identical to each other;
   nested dissection / envelope on ladybug, a forced pinv pass.
5. w = 0: three cameras that start at w = 0 stay there under FD and move under
   analytic Jacobians (jac_ref.e2e_check, which the CPU LM meets alone).
6. Converged point: jac_ref.analytic_lm from the GPU's answer lowers the cost by
   at most 1e-6 relative.
7. covariance() at the bars of tests/test_gpu_covariance.py.
8. Arguments, the VLGBA_JACOBIAN default (a keyword wins over it; a context the
   planner hands to the ordered kernels stays FD), the adjuster fingerprint,
   two ranks.

Every test prints its figures before it asserts (lines starting JAC, pytest -s).
Measured on an MI355X, no bar widened: the figures are in each test's docstring.
"""
import functools
import os

import numpy as np
import pytest

import jac_ref as jr
import robust_ref as rr
from test_gpu_robust import _problem, _same, _scene, _solve

pytestmark = pytest.mark.gpu


def _make(gpu, K, pt, cam, ox, n, na, env=None, **kw):
    """A context created with the environment variables env set (they are read
    at vlgba_create), restored afterwards."""
    env = dict(env or {})
    old = {k: os.environ.pop(k, None) for k in env}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        return gpu.BundleAdjuster(K, pt, cam, ox, n, na, **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------------------
# 1. stage
# ---------------------------------------------------------------------------
STAGE = [("banded", 6, {}), ("banded", 7, {}), ("banded", 10, {}), ("banded", 12, {}),
         ("long", 6, {}), ("ladder", 7, {}), ("ladder", 10, {}), ("ladder", 12, {}),
         ("banded", 6, dict(pivot="first2")), ("banded", 6, dict(fix_structure=True))]


@pytest.mark.parametrize("name,na,opt", STAGE,
                         ids=[f"{n}{a}" + "".join("-" + o for o in sorted(q))
                              for n, a, q in STAGE])
def test_linearisation_within_the_reference_bounds(gpu, name, na, opt):
    """Measured, largest |diff| / bound over all cases: U 0.12, eA 0.059, V 0.17,
    eB 0.16, W 0.51 (all on the num_a 12 ladder; banded num_a 6: 0.014, 0.0086,
    0.027, 0.024, 0.072).  The W bounds are 1e-11 .. 2e-8 of |W| at most; the FD
    linearisation is outside them for every nonzero W entry (1.000) in every
    case."""
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    kw = dict(kw, **opt)
    pivot = None
    if kw.get("pivot") == "first2":
        pivot = kw["pivot"] = np.arange(sc.m) < 2
    lin = {}
    for mode in ("analytic", "fd"):
        with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, na, jacobian=mode, **kw) as ba:
            assert ba.get_jacobian() == mode
            ba.set_params(a, b)
            lin[mode] = ba.linearization()
            e = ba.residuals()[0]
            plan = ba.plan_info()
    assert plan["ordered"] == 0 and (name != "long" or plan["long_points"] == 1), plan
    if name == "ladder":
        import track_scenes as ts
        assert plan["long_points"] == ts.is_long(np.bincount(pt)).sum() >= 10, plan
    R = jr.linearization(K, a, b, pt, cam, e, sc.m, sc.n, na,
                         fix_structure=bool(opt.get("fix_structure")), pivot=pivot)
    fig = {k: rr.ratio(lin["analytic"][k], R[k], R[k + "_b"]) for k in ("U", "eA", "V", "eB", "W")}
    Wref, Wb = np.asarray(R["W"], dtype=np.float64), np.asarray(R["W_b"], dtype=np.float64)
    nz = Wref != 0
    out = np.abs(lin["fd"]["W"].astype(jr.LD) - R["W"]) > R["W_b"]
    frac = float(out[nz].mean()) if nz.any() else float("nan")
    rel = float((Wb[nz] / np.abs(Wref[nz])).max()) if nz.any() else float("nan")
    print(f"JAC stage {name} num_a {na} {sorted(opt)}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f"; FD outside the W bound for {frac:.3f} of {int(nz.sum())} nonzero entries "
          f"(largest W bound / |W| {rel:.2e})")
    assert all(v <= 1.0 for v in fig.values()), fig
    if opt.get("fix_structure"):
        assert all(np.all(lin["analytic"][k] == 0) for k in ("V", "eB", "W"))
        assert np.any(lin["analytic"]["U"] != 0)
    else:
        assert frac > 0.5, frac
    if pivot is not None:
        L = lin["analytic"]
        assert np.all(L["U"][:, :, pivot] == 0) and np.all(L["eA"][:, pivot] == 0)
        assert np.all(L["W"][:, :, pivot[cam]] == 0) and np.any(L["W"] != 0)


# ---------------------------------------------------------------------------
# 2. what must not move
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,na", [("banded", 6), ("banded", 10), ("banded", 12), ("long", 6)])
def test_residuals_and_cost_are_the_same_bits(gpu, name, na):
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    res = {}
    for mode in ("fd", "analytic"):
        with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, na, jacobian=mode, **kw) as ba:
            ba.set_params(a, b)
            e = ba.residuals()[0]
            info = ba.step(relinearize=True, update_lm=False)
            res[mode] = (e, info.old_sse, info.new_sse)
    print(f"JAC same bits {name} num_a {na}: old_sse fd {res['fd'][1]!r} analytic "
          f"{res['analytic'][1]!r}; new_sse {res['fd'][2]:.10g} / {res['analytic'][2]:.10g}")
    assert np.array_equal(res["fd"][0], res["analytic"][0])
    assert res["fd"][1] == res["analytic"][1]
    assert res["fd"][2] != res["analytic"][2]      # another step: the Jacobians differ


@pytest.mark.parametrize("name,na", [("banded", 6), ("banded", 7), ("long", 6)])
def test_set_jacobian_fd_restores_the_default_solver(gpu, name, na):
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    args = (K, pt, cam, ox, sc.n, na)
    with gpu.BundleAdjuster(*args, **kw) as ba:
        assert ba.get_jacobian() == "fd"
        fresh = _solve(ba, a, b)
    with gpu.BundleAdjuster(*args, jacobian="analytic", **kw) as ba:
        an = _solve(ba, a, b)
        ba.set_jacobian("fd")
        assert ba.get_jacobian() == "fd"
        back = _solve(ba, a, b)
        ba.set_jacobian("analytic")
        again = _solve(ba, a, b)
    print(f"JAC restore {name} num_a {na}: fd {fresh[3][0]} passes error_ {fresh[0][-1]:.10g}; "
          f"analytic {an[3][0]} passes error_ {an[0][-1]:.10g}")
    assert fresh[3][1] >= 2 and an[3][1] >= 2
    assert _same(back, fresh), (back[0], fresh[0], back[3], fresh[3])
    assert _same(again, an), (again[0], an[0])
    assert not np.array_equal(an[1], fresh[1])


# ---------------------------------------------------------------------------
# 3. fused against VLGBA_FUSED=0; the LOSS x JAC instantiations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,na", [("banded", 6), ("banded", 10), ("banded", 12), ("long", 6)])
def test_fused_equals_unfused(gpu, name, na):
    """tests/test_gpu_fused.py's comparison in analytic mode, at its bars: the
    applied step and the linearisation at the new point bit-identical, the old
    cost too; the new cost and dp'(lambda dp + g) to summation order."""
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    res = {}
    for fused in (True, False):
        with _make(gpu, K, pt, cam, ox, sc.n, na, env={"VLGBA_FUSED": None if fused else "0"},
                   jacobian="analytic", **kw) as ba:
            ba.set_params(a, b)
            i1 = ba.step(relinearize=False, update_lm=True)
            da, db = ba.last_step()
            res[fused] = (i1, da.copy(), db.copy(), ba.get_params(), ba.linearization(),
                          ba.plan_info())
    (fi, ui), f, u = (res[True][0], res[False][0]), res[True], res[False]
    print(f"JAC fused {name} num_a {na}: cost {fi.old_sse:.10g} -> {fi.new_sse:.10g}, new cost "
          f"rel diff {abs(fi.new_sse - ui.new_sse) / ui.new_sse:.2e}, dpg rel diff "
          f"{abs(fi.dpg - ui.dpg) / abs(ui.dpg):.2e}")
    assert fi.accepted == 1 and ui.accepted == 1
    assert fi.old_sse == ui.old_sse
    assert abs(fi.new_sse - ui.new_sse) <= 1e-13 * ui.new_sse, (fi.new_sse, ui.new_sse)
    assert abs(fi.dpg - ui.dpg) <= 1e-12 * abs(ui.dpg), (fi.dpg, ui.dpg)
    assert np.array_equal(f[1], u[1]) and np.array_equal(f[2], u[2])
    assert np.array_equal(f[3][0], u[3][0]) and np.array_equal(f[3][1], u[3][1])
    for nm in ("W", "V", "eB", "U", "eA"):
        assert np.array_equal(f[4][nm], u[4][nm]), (name, nm)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name,na", [("banded", 6), ("banded", 7), ("banded", 10),
                                     ("banded", 12), ("long", 6)])
def test_huber_1e150_is_bit_identical_to_no_loss(gpu, name, na, fused):
    sc, pt, cam, ox = _scene(name, na)
    K, a, b, kw = _problem(sc, na)
    env = {"VLGBA_FUSED": None if fused else "0"}
    with _make(gpu, K, pt, cam, ox, sc.n, na, env=env, jacobian="analytic", **kw) as ba:
        plain = _solve(ba, a, b)
    with _make(gpu, K, pt, cam, ox, sc.n, na, env=env, jacobian="analytic", loss="huber",
               loss_scale=1e150, **kw) as ba:
        huge = _solve(ba, a, b)
        ba.set_loss("cauchy", 3.0)
        cauchy = _solve(ba, a, b)
    print(f"JAC loss identity {name} num_a {na} fused {fused}: {plain[3][0]} passes, error_ "
          f"{plain[0][0]:.6g} -> {plain[0][-1]:.6g}; cauchy -> {cauchy[0][-1]:.6g}")
    assert plain[3][1] >= 2, plain[3]
    assert _same(huge, plain), (huge[0], plain[0], huge[3], plain[3])
    assert not np.array_equal(cauchy[0], plain[0])


# ---------------------------------------------------------------------------
# 4. solvers
# ---------------------------------------------------------------------------
def test_cyclic_reduction_with_and_without_the_folded_camera_update(gpu):
    sc, pt, cam, ox = _scene("banded", 6)
    K, a, b, kw = _problem(sc, 6)
    res = {}
    for fold in (True, False):
        with _make(gpu, K, pt, cam, ox, sc.n, 6, env={"VLGBA_CAMUPD_FOLD": None if fold else "0"},
                   jacobian="analytic") as ba:
            res[fold] = _solve(ba, a, b)
            plan = ba.plan_info()
        assert plan["cr_levels"] > 0 and plan["camupd_fold"] == int(fold), plan
    err, st = res[True][0], res[True][3]
    print(f"JAC cyclic reduction: cr_levels {plan['cr_levels']} error_ {err[0]:.6g} -> "
          f"{err[-1]:.10g} in {st[0]} passes")
    assert st[4] == 0 and st[1] >= 2 and np.all(np.diff(err) < 0)
    assert _same(res[True], res[False])


def test_nested_dissection_on_ladybug(gpu):
    sc, pt, cam, ox = _scene("ladybug", 6)
    K, a, b, kw = _problem(sc, 6)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, jacobian="analytic") as ba:
        err, _, _, st = _solve(ba, a, b)
        plan = ba.plan_info()
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6) as ba:
        err_fd = _solve(ba, a, b)[0]
    print(f"JAC ladybug: cr_levels {plan['cr_levels']} nd_arcs {plan['nd_arcs']} error_ "
          f"{err[0]:.6g} -> {err[-1]:.10g} in {st[0]} passes (fd: {err_fd[-1]:.10g})")
    assert plan["cr_levels"] == 0, plan
    assert st[4] == 0 and st[1] >= 2 and np.all(np.isfinite(err)) and err[-1] < err[0]
    assert err[0] == err_fd[0]                        # the same first cost, bit for bit


def test_pinv_pass_lowers_the_cost(gpu):
    sc, pt, cam, ox = _scene("banded", 6)
    K, a, b, kw = _problem(sc, 6)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, 6, jacobian="analytic") as ba:
        ba.set_params(a, b)
        ba.force_status(4, 1)
        info = ba.step(relinearize=True, update_lm=True)
    print(f"JAC pinv pass: cost {info.old_sse:.8g} -> {info.new_sse:.8g}")
    assert info.pinv == 1 and info.accepted == 1 and info.new_sse < info.old_sse


# ---------------------------------------------------------------------------
# 5. w = 0, 6. the converged point
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    """The w = 0 scene, its dense form and the CPU analytic LM from its start."""
    s = jr.e2e_scene()
    X = np.zeros((2, s["n"], s["m"]), order="F")
    X[0, s["pt"], s["cam"]], X[1, s["pt"], s["cam"]] = s["obs_x"][:, 0], s["obs_x"][:, 1]
    vis = np.zeros((s["n"], s["m"]), order="F")
    vis[s["pt"], s["cam"]] = 1.0
    cpu = jr.analytic_lm(s["K"], s["a0"], s["b0"], X, vis, pivot=s["pivot"], **jr.E2E["stop"],
                         **jr.E2E["lm"])
    return s, X, vis, cpu


def _e2e_run(gpu, mode):
    s = _e2e()[0]
    with gpu.BundleAdjuster(s["K"], s["pt"], s["cam"], s["obs_x"], s["n"], 6, pivot=s["pivot"],
                            jacobian=mode, **jr.E2E["stop"]) as ba:
        return _solve(ba, s["a0"], s["b0"])


def test_cameras_at_w_zero_rotate(gpu, oracle):
    """Measured: FD leaves the three rotations at exactly 0 and ends at error_
    13.400893 after 67 passes; analytic moves them to |w| >= 0.0658, within
    2.1e-3 rad of the truth, error_ 0.3513106116 after 20 passes (the CPU
    analytic LM: 0.3513106116, relative difference 9.5e-16).  The zeroed
    camera's U, eA, W: 0.0097, 0.010, 0.16 of jac_ref's bounds."""
    s, X, vis, cpu = _e2e()
    fd, an = _e2e_run(gpu, "fd"), _e2e_run(gpu, "analytic")
    fig = jr.e2e_figures(s, fd[1], fd[0], an[1], an[0])
    rel = abs(an[0][-1] - cpu[2][-1]) / cpu[2][-1]
    print("JAC w = 0: FD leaves |w| %.3g; analytic moves them to |w| >= %.4f, within %.2e of "
          "the truth; error_ FD %.8g analytic %.10g" % fig
          + f"; CPU analytic LM {cpu[2][-1]:.10g} (rel diff {rel:.2e}); passes fd {fd[3][0]} "
          f"analytic {an[3][0]}")
    jr.e2e_check(fig)
    assert np.all(fd[1][0:3, s["zero"]] == 0.0)
    assert rel <= 1e-6, rel
    # one such camera's rotation columns: FD exact zeros, analytic jac_ref's
    z = int(s["zero"][0])
    lin = {}
    for mode in ("fd", "analytic"):
        with gpu.BundleAdjuster(s["K"], s["pt"], s["cam"], s["obs_x"], s["n"], 6,
                                jacobian=mode) as ba:
            ba.set_params(s["a0"], s["b0"])
            lin[mode] = ba.linearization()
            e = ba.residuals()[0]
    R = jr.linearization(s["K"], s["a0"], s["b0"], s["pt"], s["cam"], e, s["m"], s["n"], 6)
    oz = s["cam"] == z
    fig = {k: rr.ratio(lin["analytic"][k], R[k], R[k + "_b"]) for k in ("U", "eA", "W")}
    print(f"JAC w = 0 camera {z}: largest |diff| / bound " +
          " ".join(f"{k} {v:.3g}" for k, v in fig.items()) +
          f"; largest |W| rotation row analytic {np.abs(lin['analytic']['W'][0:3][:, :, oz]).max():.4g}")
    assert np.all(lin["fd"]["W"][0:3][:, :, oz] == 0) and np.all(lin["fd"]["U"][0:3, :, z] == 0)
    assert np.all(lin["fd"]["eA"][0:3, z] == 0)
    assert np.all(np.abs(np.asarray(R["W"], dtype=np.float64)[0:3][:, :, oz]).max(axis=(0, 1)) > 0)
    assert all(v <= 1.0 for v in fig.values()), fig


def test_converged_point_survives_the_reference_restart(gpu, oracle):
    """The project's restart bar (tests/test_gpu_converged.py): at most 1e-6.
    Measured: the CPU analytic LM started at the GPU's analytic answer
    (error_ 0.351310611625 after 20 passes) lowers the cost by 3.7e-14 relative;
    the two finals from the common start differ by 9.5e-16 relative.  (Under FD
    the restart figures are 1e-8 .. 1e-7: DESIGN.md sec. 3.)"""
    s, X, vis, cpu = _e2e()
    an = _e2e_run(gpu, "analytic")
    N = float(len(s["pt"]))
    e_at = oracle.mex1(s["K"], an[1], an[2], X, vis)[3][:, s["pt"], s["cam"]].T
    c_at = rr.cost_of(e_at, "none", 1.0) / N
    _, _, e_r = jr.analytic_lm(s["K"], an[1], an[2], X, vis, pivot=s["pivot"],
                               **jr.E2E["stop"], **jr.E2E["lm"])
    final = e_r[-1] if len(e_r) else c_at
    drop = (c_at - final) / c_at
    direct = abs(an[0][-1] - cpu[2][-1]) / cpu[2][-1]
    print(f"JAC converged: GPU {an[0][0]:.8g} -> {an[0][-1]:.12g} in {an[3][0]} passes; "
          f"reference cost there {c_at:.12g}; analytic_lm from there {final:.12g} (drop "
          f"{drop:.2e}); CPU LM from the common start {cpu[2][-1]:.12g} (rel diff {direct:.2e})")
    assert abs(c_at - an[0][-1]) <= 1e-12 * c_at
    assert -1e-12 <= drop <= 1e-6, drop


# ---------------------------------------------------------------------------
# 7. covariance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("na", [6, 10])
def test_covariance(gpu, na):
    """tests/test_gpu_covariance.py's camera stage, point stage and end-to-end
    check with its references fed the analytic linearisation, at its bars."""
    import cov_ref as cr
    import schur_ref as sr
    import test_gpu_covariance as tc
    sc, pt, cam, ox = _scene("banded", na)
    K, a, b, kw = _problem(sc, na)
    with gpu.BundleAdjuster(K, pt, cam, ox, sc.n, na, pivot=np.arange(sc.m) < 2,
                            jacobian="analytic", **kw) as ba:
        ba.set_params(a, b)
        lin = ba.linearization()
        cov = ba.covariance(scale=False, full=True)
    key = f"jacobian-analytic-banded{na}"
    r = dict(lin=lin, na=na, m=sc.m, n=sc.n, pt=pt, cam=cam)
    ref = tc._camera_ref(r, key)
    full, fixed = cov["full"], ref["fixed"]
    fig_full = cr.block_figure(full, ref["want"], na)
    fig_diag = cr.block_figure(cov["cam"], cr.diag_blocks(ref["want"], na), na)
    pref, bound = cr.point_cov(na, pt, cam, lin["W"], ref["Vi"], full)
    ratio = cr.point_ratio(cov["pts"], pref, bound)
    seen = np.bincount(pt, minlength=sc.n) > 0
    full_a, full_b, _ = cr.normal_inverse(na, sc.m, sc.n, pt, cam, lin["U"], lin["V"], lin["W"],
                                          fixed, seen)
    b64 = cr.point_cov_fp64(na, pt, cam, lin["W"], ref["Vi"], ref["inv64"])
    floor_a, floor_b = cr.block_figure(ref["inv64"], full_a, na), cr.block_figure(b64, full_b, 3)
    fig_a, fig_b = cr.block_figure(full, full_a, na), cr.block_figure(cov["pts"], full_b, 3)
    print(f"JAC covariance num_a {na}: fixed rows {int(fixed.sum())} cond(S0) {ref['cond']:.2g}; "
          f"cameras: diagonal blocks GPU {fig_diag:.3g} numpy {ref['floor_diag']:.3g}, all "
          f"blocks GPU {fig_full:.3g} numpy {ref['floor_full']:.3g}; points {ratio:.3g} of the "
          f"bound; end to end cameras {fig_a:.3g} floor {floor_a:.3g}, points {fig_b:.3g} floor "
          f"{floor_b:.3g}")
    assert np.array_equal(full, full.T) and np.all(np.isfinite(full))
    assert np.all(full[fixed, :] == 0.0) and cov["fixed_rows"] == int(fixed.sum()) == 2 * na
    assert fig_diag <= 8 * ref["floor_diag"] and fig_full <= 8 * ref["floor_full"]
    assert ratio <= 1.0, ratio
    assert fig_a <= 8 * floor_a and fig_b <= 8 * floor_b


# ---------------------------------------------------------------------------
# 8. arguments, the environment default, the fingerprint, two ranks
# ---------------------------------------------------------------------------
def test_arguments(gpu):
    sc, pt, cam, ox = _scene("banded", 6)
    K, a, b, kw = _problem(sc, 6)
    L = gpu.lib()
    args = (K, pt, cam, ox, sc.n, 6)
    with gpu.BundleAdjuster(*args) as ba:
        ba.set_params(a, b)
        for kind in (-1, 2, 99):
            assert L.vlgba_set_jacobian(ba._h, kind) == -1001
        assert ba.get_jacobian() == "fd"                 # a refused call changes nothing
        with pytest.raises(ValueError):
            ba.set_jacobian("central")
        ba.set_jacobian("analytic")
        assert ba.get_jacobian() == "analytic"
    with pytest.raises(ValueError):
        gpu.BundleAdjuster(*args, jacobian="central")
    for mode in (dict(parity=True), dict(ordered=True)):
        with gpu.BundleAdjuster(*args, **mode) as ba:
            assert L.vlgba_set_jacobian(ba._h, 1) == -1001
            assert L.vlgba_set_jacobian(ba._h, 0) == -1001
            assert ba.get_jacobian() == "fd"
        with pytest.raises(ValueError):
            gpu.BundleAdjuster(*args, jacobian="analytic", **mode)
    # the environment default: fast-path contexts only
    with _make(gpu, *args, env={"VLGBA_JACOBIAN": "analytic"}) as ba:
        assert ba.get_jacobian() == "analytic"
        ba.set_params(a, b)
        env_lin = ba.linearization()
    with gpu.BundleAdjuster(*args, jacobian="analytic") as ba:
        ba.set_params(a, b)
        kw_lin = ba.linearization()
    assert all(np.array_equal(env_lin[k], kw_lin[k]) for k in env_lin)
    with _make(gpu, *args, env={"VLGBA_JACOBIAN": "analytic"}, parity=True) as ba:
        assert ba.get_jacobian() == "fd"
    with _make(gpu, *args, env={"VLGBA_JACOBIAN": "fd"}) as ba:
        assert ba.get_jacobian() == "fd"
    # a keyword wins over the environment, in both directions
    with _make(gpu, *args, env={"VLGBA_JACOBIAN": "analytic"}, jacobian="fd") as ba:
        assert ba.get_jacobian() == "fd"
        ba.set_params(a, b)
        fd_lin = ba.linearization()
    with gpu.BundleAdjuster(*args) as ba:
        ba.set_params(a, b)
        plain_lin = ba.linearization()
    assert all(np.array_equal(fd_lin[k], plain_lin[k]) for k in fd_lin)
    assert not np.array_equal(fd_lin["W"], env_lin["W"])
    with _make(gpu, *args, env={"VLGBA_JACOBIAN": "fd"}, jacobian="analytic") as ba:
        assert ba.get_jacobian() == "analytic"


@functools.lru_cache(maxsize=None)
def _planner_ordered():
    """A problem the planner hands to the ordered kernels although ordered == 0 is
    asked for: every point seen by all 600 cameras, 380 points -- 380 x 600 x 601
    / 2 = 6.85e7 long-track terms, above the fast path's 2^26."""
    from bundleadjustmentmatlab_amd.scene import make_config, project
    sc = make_config("cfg2", m=600, n=380, seed=9)
    pt = np.repeat(np.arange(sc.n), sc.m).astype(np.int32)
    cam = np.tile(np.arange(sc.m), sc.n).astype(np.int32)
    ox, _ = project(sc.K, sc.w, sc.T, sc.X, cam, pt)
    return sc, pt, cam, np.ascontiguousarray(ox)


def test_planner_ordered_context_stays_fd(gpu):
    """VLGBA_JACOBIAN=analytic must not reach a context that runs the ordered
    kernels: they read the rotation table's slots 1..4 as R(w + h e_k)."""
    sc, pt, cam, ox = _planner_ordered()
    K, a, b, kw = _problem(sc, 6)
    args = (K, pt, cam, ox, sc.n, 6)
    L = gpu.lib()
    lin = {}
    for env in ("analytic", None):
        with _make(gpu, *args, env={"VLGBA_JACOBIAN": env}) as ba:
            plan = ba.plan_info()
            assert plan["ordered"] == 1, plan
            assert ba.get_jacobian() == "fd"
            assert L.vlgba_set_jacobian(ba._h, 1) == -1001
            assert ba.get_jacobian() == "fd"
            ba.set_params(a, b)
            lin[env] = ba.linearization()
    print(f"JAC planner-ordered: {len(pt)} observations, plan ordered {plan['ordered']}, "
          f"largest |W| {np.abs(lin[None]['W']).max():.4g}")
    assert all(np.array_equal(lin["analytic"][k], lin[None][k]) for k in lin[None])
    assert np.all(np.isfinite(lin[None]["U"])) and np.any(lin[None]["W"] != 0)
    with pytest.raises(gpu.VlgbaError, match="-1001"):
        _make(gpu, *args, jacobian="analytic")


def test_drivers_and_the_fingerprint(gpu):
    from bundleadjustmentmatlab_amd.bundle import euclid_obs_adjuster
    s = jr.e2e_scene()
    sc_args = (s["K"], s["a0"][3:6], s["a0"][0:3], np.vstack([s["b0"], np.ones((1, s["n"]))]))
    obs = (s["pt"], s["cam"], s["obs_x"])
    fd = gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration")[4]
    an = gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration", jacobian="analytic")[4]
    assert fd[0] == an[0] and an[-1] < fd[-1]
    pre = euclid_obs_adjuster(s["K"], s["m"], s["n"], *obs, "fix_calibration", jacobian="analytic")
    assert pre.get_jacobian() == "analytic"
    again = gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration", jacobian="analytic",
                                  adjuster=pre)[4]
    assert np.array_equal(again, an)
    pre = euclid_obs_adjuster(s["K"], s["m"], s["n"], *obs, "fix_calibration", jacobian="analytic")
    with pytest.raises(ValueError):      # built for the other mode
        gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration", jacobian="fd", adjuster=pre)
    # the fingerprint is the context's own mode, whatever set it
    old = os.environ.get("VLGBA_JACOBIAN")
    os.environ["VLGBA_JACOBIAN"] = "analytic"
    try:
        env_fd = euclid_obs_adjuster(s["K"], s["m"], s["n"], *obs, "fix_calibration",
                                     jacobian="fd")
        env_default = euclid_obs_adjuster(s["K"], s["m"], s["n"], *obs, "fix_calibration")
    finally:
        os.environ.pop("VLGBA_JACOBIAN")
        if old is not None:
            os.environ["VLGBA_JACOBIAN"] = old
    assert env_fd.get_jacobian() == "fd" and env_fd.fingerprint[-1] == "fd"
    assert env_default.get_jacobian() == "analytic" and env_default.fingerprint[-1] == "analytic"
    env_fd.close()
    with pytest.raises(ValueError):
        gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration", jacobian="fd",
                              adjuster=env_default)
    with pytest.raises(ValueError):
        gpu.bundle_euclid_obs(*sc_args, *obs, "fix_calibration", jacobian="analytic", parity=True)
    # the projective driver takes it too
    from bundleadjustmentmatlab_amd.scene import projective_from
    scb, pt, cam, ox = _scene("banded", 12)
    Pp, Xp = projective_from(scb)
    pf = gpu.bundle_projective_obs(Pp, Xp, pt, cam, ox)[2]
    pa = gpu.bundle_projective_obs(Pp, Xp, pt, cam, ox, jacobian="analytic")[2]
    print(f"JAC drivers: euclid error_ fd {fd[-1]:.8g} analytic {an[-1]:.8g}; projective fd "
          f"{pf[-1]:.8g} analytic {pa[-1]:.8g}")
    assert pf[0] == pa[0] and not np.array_equal(pf, pa) and pa[-1] < pa[0]


def test_two_rank_threads_match_one_rank(gpu):
    """tests/test_gpu_robust.py's two-rank comparison (the bars of
    tests/test_gpu_dist.py) in analytic mode."""
    import threading
    from bundleadjustmentmatlab_amd.dist import HostGroup
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=40, n=5000, seed=21)
    K, a, b, kw = _problem(sc, 6)
    args = (K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6)

    def passes(ba):
        assert ba.get_jacobian() == "analytic"
        ba.set_params(a, b)
        infos = [ba.step(relinearize=True, update_lm=True) for _ in range(3)]
        return ([i.old_sse for i in infos], [i.new_sse for i in infos],
                [i.accepted for i in infos], ba.plan_info())

    with gpu.BundleAdjuster(*args, jacobian="analytic") as ba:
        one = passes(ba)
    world = 2
    grp = HostGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            with gpu.BundleAdjuster(*args, rank=r, world_size=world,
                                    allreduce=grp.allreduce_fn(r), jacobian="analytic") as ba:
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
    print(f"JAC two ranks: old {old} new {new} | one rank old {one[0]} new {one[1]}")
    assert acc == one[2] and sum(acc) >= 2
    assert abs(old[0] - one[0][0]) <= 1e-11 * one[0][0]
    assert abs(new[0] - one[1][0]) <= 1e-7 * one[1][0]
    assert np.allclose(old, one[0], rtol=1e-4, atol=0)
    assert np.allclose(new, one[1], rtol=1e-4, atol=0)
