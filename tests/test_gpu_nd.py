"""The envelope Cholesky on a nested-dissection camera order (ba_chol_plan.cpp's
planner; ba_chol.hip: k_factor_multi, k_sep_update / k_sep_reduce,
k_nd_scatter).  The cameras split into arcs of consecutive cameras and a
separator (cameras co-visible with an earlier arc); the arcs' columns are
factored side by side, then the separator.  A different elimination order
than the natural envelope, so the reduced solve agrees with it to rounding
(not bit for bit); every other quantity of the pass is the same.

The reduced solve is checked against the natural-order envelope Cholesky
(itself bit-identical to the dense tile Cholesky, test_gpu_parity.py) on the
same pass: relative error of da within 1e-9 (the systems here have condition
numbers near 1e4 after the damping), and whole LM runs within the north
star's 1e-6 relative.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _scene(kind, m, seed):
    from bundleadjustmentmatlab_amd.scene import make_config
    if kind == "ladybug":
        return make_config("ladybug", m=m, n=100 * m, seed=seed)
    return make_config("cfg2", m=m, n=80 * m, seed=seed)


def _params(sc, num_a):
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    return a, np.asfortranarray(sc.X0[:3])


def _pass(gpu, sc, num_a, solver, timing=False):
    a, b = _params(sc, num_a)
    with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a,
                            solver=solver) as ba:
        ba.set_params(a, b)
        ba.set_timing(timing)
        info = ba.step(relinearize=True, update_lm=False)
        da, db = ba.last_step()
        plan = ba.plan_info()
        km = ba.kernel_ms() if timing else {}
    return info, da.copy(), db.copy(), plan, km


@pytest.mark.parametrize("kind,m,num_a", [("ladybug", 120, 6), ("ladybug", 300, 6),
                                          ("cfg2", 60, 6), ("ladybug", 90, 7),
                                          ("ladybug", 80, 10)])
def test_nd_solve_matches_envelope(gpu, kind, m, num_a):
    sc = _scene(kind, m, seed=3)
    env, da0, db0, p0, _ = _pass(gpu, sc, num_a, "envelope")
    nd, da1, db1, p1, km = _pass(gpu, sc, num_a, "nd", timing=True)
    assert p0["nd_arcs"] == 0 and p1["nd_arcs"] >= 2, p1
    assert p1["cr_levels"] == 0
    assert "k_factor_step" in km          # k_factor_multi and the separator's columns
    assert env.old_sse == nd.old_sse
    assert env.chol_failed == 0 and nd.chol_failed == 0
    scale = np.max(np.abs(da0))
    assert np.max(np.abs(da1 - da0)) <= 1e-9 * scale, np.max(np.abs(da1 - da0)) / scale
    assert np.max(np.abs(db1 - db0)) <= 1e-9 * np.max(np.abs(db0))
    assert abs(nd.new_sse - env.new_sse) <= 1e-9 * env.new_sse


def test_nd_separator_update_timed(gpu):
    """A split with a separator runs the SYRK launches (timed as k_syrk)."""
    sc = _scene("ladybug", 300, seed=4)
    _, _, _, plan, km = _pass(gpu, sc, 6, "nd", timing=True)
    assert plan["nd_arcs"] >= 2 and plan["nd_sep_tiles"] > 0, plan
    assert "k_syrk" in km, km


def test_nd_lm_trajectory(gpu):
    """Whole LM runs: the nested-dissection order ends where the natural one
    does.  The first step's cost agrees to 1e-9; later steps start from
    slightly different points and the slow tail of this scene amplifies the
    difference (1e-8 relative by iteration 4), so the rest is held to the
    north star's 1e-6 relative -- on the costs, not on the pass counts: where
    the stop rule fires in a tail of near-equal decrements is a matter of the
    last bits (once 15 vs 11 passes, costs within the bar)."""
    sc = _scene("ladybug", 200, seed=9)
    out = {}
    for solver in ("envelope", "nd"):
        a, b = _params(sc, 6)
        with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, solver=solver,
                                stop_rel=1e-9, max_iter=15) as ba:
            ba.set_params(a, b)
            err, st = ba.run()
            out[solver] = (err.copy(), st)
    e0, e1 = out["envelope"][0], out["nd"][0]
    n = min(len(e0), len(e1))
    assert n >= 3, (e0, e1)
    assert np.allclose(e0[:2], e1[:2], rtol=1e-9, atol=0)
    assert np.allclose(e0[:n], e1[:n], rtol=1e-6, atol=0), (e1[:n] - e0[:n]) / e0[:n]
    assert abs(e0[-1] - e1[-1]) <= 1e-6 * e0[-1], (e0[-1], e1[-1], len(e0), len(e1))


def test_nd_auto_takes_it_when_it_pays(gpu):
    """auto: a long banded sequence with loop closures is not tile-tridiagonal
    (no cyclic reduction) and the split shortens the step chain by more than
    a quarter, so the nested-dissection order is used; VLGBA_ND=0 keeps the
    natural order."""
    import os
    sc = _scene("ladybug", 400, seed=5)
    _, da1, _, p1, _ = _pass(gpu, sc, 6, "auto")
    os.environ["VLGBA_ND"] = "0"
    try:
        _, da0, _, p0, _ = _pass(gpu, sc, 6, "auto")
    finally:
        del os.environ["VLGBA_ND"]
    assert p1["cr_levels"] == 0 and p1["nd_arcs"] >= 2, p1
    assert p0["nd_arcs"] == 0
    assert np.max(np.abs(da1 - da0)) <= 1e-9 * np.max(np.abs(da0))


def test_nd_spin_timeout_resolves_bit_identically(gpu, monkeypatch):
    """The one-launch backward solve's hand-off timeout on the
    nested-dissection order: the re-solve with per-column k_backward gives the
    same result bit for bit."""
    sc = _scene("ladybug", 150, seed=7)
    a, b = _params(sc, 6)

    def run():
        with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, solver="nd",
                                stop_rel=1e-9, max_iter=12) as ba:
            ba.set_params(a, b)
            err, st = ba.run()
            return err.copy(), st, [x.copy() for x in ba.get_params()]
    e0, s0, p0 = run()
    monkeypatch.setenv("VLGBA_DEBUG_SPIN_TIMEOUT", "0:3")
    e1, s1, p1 = run()
    assert s0.spin_retries == 0 and s1.spin_retries == 3
    assert np.array_equal(e0, e1)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


@pytest.mark.parametrize("kind,m,num_a", [("ladybug", 300, 6), ("ladybug", 90, 7)])
def test_nd_grouped_order_bit_identical(gpu, monkeypatch, kind, m, num_a):
    """k_factor_multi's workgroups grouped by role (every arc's diagonal
    workgroup, then the panels, then the trailing pairs: the default) against
    the arc-major order (VLGBA_ND_GROUPED=0): the same roles, so whole LM runs
    agree bit for bit."""
    sc = _scene(kind, m, seed=6)
    a, b = _params(sc, num_a)

    def run():
        with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, solver="nd",
                                stop_rel=1e-9, max_iter=8) as ba:
            ba.set_params(a, b)
            ba.step(relinearize=True, update_lm=False)
            da, db = ba.last_step()
            err, st = ba.run()
            return da.copy(), err.copy(), [x.copy() for x in ba.get_params()], ba.plan_info()
    da0, e0, p0, plan = run()
    monkeypatch.setenv("VLGBA_ND_GROUPED", "0")
    da1, e1, p1, _ = run()
    assert plan["nd_arcs"] >= 2, plan
    assert np.array_equal(da0, da1)
    assert np.array_equal(e0, e1)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


@pytest.mark.parametrize("solver,m,num_a", [("nd", 300, 6), ("envelope", 300, 6),
                                             ("nd", 90, 7), ("envelope", 120, 10)])
def test_env_runner_bit_identical(gpu, monkeypatch, solver, m, num_a):
    """Runner mode (opt-in, VLGBA_ENV_RUNNER=1: k_env_runner, one persistent
    workgroup per arc on the side stream, factors the diagonal tiles and forms
    each column's first panel tile while the column launches run the other
    panels and the trailing updates; the tiles they exchange go through sc1
    stores and flags) against the column launches alone: the same operations
    in the same order on every tile, so whole LM runs agree bit for bit, and
    no hand-off gives up (no re-solve).  The context's runner-launch count
    proves the runner really ran (a runner switched off earlier in the
    process would otherwise make this test compare the launches with
    themselves).  fail_starts: the first starts of the runner fail
    (vlgba_debug_force_status word 6) -- those factorizations run with the
    column launches alone, bit for bit the same."""
    sc = _scene("ladybug", m, seed=12)
    a, b = _params(sc, num_a)

    def run(fail_starts=0):
        with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a,
                                solver=solver, stop_rel=1e-9, max_iter=8) as ba:
            if fail_starts:
                ba.force_status(6, fail_starts)
            ba.set_params(a, b)
            ba.step(relinearize=True, update_lm=False)
            da, db = ba.last_step()
            err, st = ba.run()
            return (da.copy(), err.copy(), st, [x.copy() for x in ba.get_params()],
                    ba.plan_info()["env_runner_runs"])
    monkeypatch.delenv("VLGBA_ENV_RUNNER", raising=False)   # the default: off
    da0, e0, s0, p0, r0 = run()
    monkeypatch.setenv("VLGBA_ENV_RUNNER", "1")
    monkeypatch.setenv("VLGBA_ENV_RUNNER_MIN", "1")   # these runs are short
    da1, e1, s1, p1, r1 = run()
    da2, e2, s2, p2, r2 = run(fail_starts=2)
    assert r0 == 0 and r1 > 0 and 0 <= r2 < r1, (r0, r1, r2)
    assert s0.spin_retries == 0 and s1.spin_retries == 0 and s2.spin_retries == 0
    for da, e, p in ((da1, e1, p1), (da2, e2, p2)):
        assert np.array_equal(da0, da)
        assert np.array_equal(e0, e)
        assert np.array_equal(p0[0], p[0]) and np.array_equal(p0[1], p[1])


def test_nd_projective(gpu):
    """The projective camera (num_a = 12: 64-row tiles hold 5 1/3 cameras, so
    cameras straddle tiles inside every part) on the nested-dissection order,
    at the reference's lambda0 = 1e-3 (bundle_projective.m:86).  The damped S
    keeps the projective gauge's near-null directions (15 per scene), so its
    condition number is large (2.3e13 on this scene): each order's da must be
    a backward-stable solve of the same S (normwise backward error <= 1e-13,
    numpy's dense S on the host, a bar independent of cond(S)), and the two
    orders agree to 1e-9 relative as on the well-conditioned scenes (measured
    2.8e-13: their rounding errors do not line up with the near-null
    directions).  Neither order meets a non-positive pivot (no pinv step)."""
    from bundleadjustmentmatlab_amd.projective import pack_a
    from bundleadjustmentmatlab_amd.scene import projective_from
    sc = _scene("ladybug", 160, seed=12)
    Pp, Xp = projective_from(sc)
    a, b = pack_a(Pp), np.asfortranarray(Xp[0:3])
    out = {}
    for solver in ("envelope", "nd"):
        with gpu.BundleAdjuster(None, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 12, m=sc.m,
                                model="projective", solver=solver, lambda0=1e-3) as ba:
            ba.set_params(a, b)
            S, e = ba.reduced_system(dense=True)
            info = ba.step(relinearize=False, update_lm=False)
            da, db = ba.last_step()
            out[solver] = (info, da.reshape(-1, order="F").copy(), db.copy(), ba.plan_info(),
                           np.tril(S) + np.tril(S, -1).T, e.reshape(-1).copy())
    (e0, da0, db0, p0, S, rhs), (e1, da1, db1, p1, S1, _) = out["envelope"], out["nd"]
    assert p0["nd_arcs"] == 0 and p1["nd_arcs"] >= 2
    assert np.array_equal(S, S1)
    assert e0.old_sse == e1.old_sse and e0.chol_failed == 0 and e1.chol_failed == 0
    cond = np.linalg.cond(S)
    nS = np.linalg.norm(S, 2)
    for d in (da0, da1):
        bwd = np.linalg.norm(S @ d - rhs) / (nS * np.linalg.norm(d) + np.linalg.norm(rhs))
        assert bwd <= 1e-13, bwd
    bar = 1e-9
    rel = np.linalg.norm(da1 - da0) / np.linalg.norm(da0)
    print(f"projective ND: cond(S) {cond:.2e}, da relative difference {rel:.2e} (bar {bar:.1e})")
    assert rel <= bar, (rel, cond)
    assert np.linalg.norm(db1 - db0) <= bar * np.linalg.norm(db0)


@pytest.mark.parametrize("solver", ["envelope", "nd"])
def test_envelope_factor_bit_identical_under_load(gpu, solver):
    """The envelope factor's workgroups of one tile column must not depend on
    being resident together: with another stream keeping the GPU busy, the
    column's workgroups start at different times.  Workgroup 0 used to store
    L_kk over A_kk, which a late panel workgroup then factored again (a
    non-positive pivot or a wrong panel: run-to-run differences and pinv steps
    of the growing replay, tools/solve_stress.py).  Every pass under load
    equals the idle pass bit for bit."""
    import threading

    import torch
    sc = _scene("ladybug", 300, seed=3)
    a, b = _params(sc, 6)
    with gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6,
                            solver=solver) as ba:
        ba.set_params(a, b)
        info0 = ba.step(relinearize=True, update_lm=False)
        da0 = ba.last_step()[0].copy()
        assert not info0.chol_failed and not info0.pinv
        stop = threading.Event()

        def burn():
            s = torch.cuda.Stream()
            x = torch.randn(4096, 4096, device="cuda")
            with torch.cuda.stream(s):
                while not stop.is_set():
                    for _ in range(10):
                        x = torch.tanh(x @ x * 1e-4)
                    s.synchronize()
        th = threading.Thread(target=burn)
        th.start()
        try:
            bad = []
            for rep in range(40):
                info = ba.step(relinearize=True, update_lm=False)
                da = ba.last_step()[0]
                if info.chol_failed or info.pinv or not np.array_equal(da, da0):
                    bad.append((rep, bool(info.chol_failed), bool(info.pinv),
                                float(np.abs(da - da0).max())))
        finally:
            stop.set()
            th.join()
    assert not bad, bad
