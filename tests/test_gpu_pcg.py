"""The block-Jacobi PCG reduced solve (solver="pcg", vlgba_options.dense_solve = 5;
csrc/ba_pcg.hip) on the GPU, against tests/pcg_ref.py (checked on the CPU by
tests/test_pcg_ref.py) and against the envelope Cholesky of the same pass.

Small scenes, where the kernels' own branches are: ladybug at m = 40 and 120
(rows of 3 .. 40 neighbours, 10 .. 30 workgroups), cfg2 at m = 60 (a band; m
no multiple of the four rows of a workgroup at m = 1, 2), track_scenes.shared
(64): 100 cameras of which 90 are mutually co-visible, so 89 and more
neighbours in a row -- more than a wave has lanes, several rounds of every
neighbour slice -- and m = 1, m = 2 cut from cfg2; num_a 6, 7, 9, 10 and the
projective model's 12 (10, 9, 7, 6 and 5 neighbour slices per wave).

Bounds.  The stop rule's: relres <= tol as reported, and the residual
recomputed from the downloaded blocks and da in long double within 1.01 tol
(the 1 % for the recurrence's rounding, as on the CPU).  Against the direct
solve at tolerance 1e-12: 10 times the same distance of pcg_ref's fp64
solution of the downloaded blocks from their long double solution (floor
1e-12), computed here per scene -- the factor for the GPU's other summation
order.  Zero rows: exactly 0.  m = 1: one iteration at tolerance 1e-6 -- with
M = S the first step is the solution and leaves r_1 = r_0 - alpha S M^-1 r_0,
rounding of size u cond(S_11) |r_0| <= 2^-53 * 1e9 ~ 1e-7 for a damped camera
block.
"""
import dataclasses
import functools
import types

import numpy as np
import pytest

import pcg_ref

pytestmark = pytest.mark.gpu


def _params(sc, na):
    a = np.zeros((na, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if na == 7:
        a[6] = sc.K[0]
    elif na == 10:
        a[6:10] = sc.K
    return a, np.asfortranarray(sc.X0[:3])


def _cut(sc, mc):
    """The scene's first mc cameras and the points they see."""
    keep = sc.obs_cam < mc
    pts, pt = np.unique(sc.obs_pt[keep], return_inverse=True)
    return dataclasses.replace(
        sc, K=np.asfortranarray(sc.K[:, :mc]), w0=sc.w0[:, :mc],
        T0=sc.T0[:, :mc], w=sc.w[:, :mc], T=sc.T[:, :mc], X=sc.X[:, pts], X0=sc.X0[:, pts],
        obs_pt=pt.astype(np.int32), obs_cam=sc.obs_cam[keep], obs_x=sc.obs_x[keep])


def _without_camera(sc, j):
    keep = sc.obs_cam != j
    return dataclasses.replace(sc, obs_pt=sc.obs_pt[keep], obs_cam=sc.obs_cam[keep],
                               obs_x=sc.obs_x[keep])


@functools.lru_cache(maxsize=None)
def _scene(name):
    from bundleadjustmentmatlab_amd.scene import make_config
    if name == "ladybug40":
        return make_config("ladybug", m=40, n=1500, max_track=30, radius=150.0, seed=23)
    if name == "ladybug120":
        return make_config("ladybug", m=120, n=12000, max_track=30, radius=150.0, seed=23)
    if name == "cfg2":
        return make_config("cfg2", m=60, n=3000, seed=3)
    if name == "shared":
        import track_scenes as ts
        return ts.shared(C=64)[0]
    if name in ("m1", "m2"):
        return _cut(make_config("cfg2", m=13, n=400, seed=3), int(name[1]))
    if name == "noobs":   # camera 7 sees nothing
        return _without_camera(_scene("ladybug40"), 7)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name, na):
    """What a context of the scene at num_a needs (shared, never modified)."""
    sc = _scene(name)
    pt, cam, ox, K, kw = sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K, {}
    if na == 12:
        from bundleadjustmentmatlab_amd.scene import projective_from
        Pp, Xp = projective_from(sc)
        a = np.asfortranarray(Pp.reshape(12, sc.m, order="F"))
        b, K, kw = np.asfortranarray(Xp[0:3]), None, dict(model="projective", m=sc.m)
    elif na == 9:
        from test_gpu_stage_ref import _radial
        a, b, ox = _radial(sc, pt, cam)
    else:
        a, b = _params(sc, na)
    return types.SimpleNamespace(name=name, na=na, m=sc.m, n=sc.n, K=K, a=a, b=b, pt=pt, cam=cam,
                                 ox=ox, kw=kw)


def _make(gpu, c, solver, **kw):
    return gpu.BundleAdjuster(c.K, c.pt, c.cam, c.ox, c.n, c.na, solver=solver, **c.kw, **kw)


def _pass(gpu, c, solver, tol=None, max_iter=None, a=None, prepare=None, **kw):
    """One pass at the start parameters: the step info's fields, da, and for
    the PCG its statistics and the context's own blocks."""
    pcg = solver == "pcg"
    if pcg:
        kw = dict(kw, pcg_tol=tol, pcg_max_iter=max_iter)
    with _make(gpu, c, solver, **kw) as ba:
        ba.set_params(c.a if a is None else a, c.b)
        if prepare:
            prepare(ba)
        i = ba.step(relinearize=True, update_lm=False)
        out = types.SimpleNamespace(old=i.old_sse, new=i.new_sse, dpg=i.dpg, acc=i.accepted,
                                    pinv=i.pinv, da=ba.last_step()[0].copy(),
                                    plan=ba.plan_info())
        if pcg:
            out.stats = ba.pcg_stats()
            out.sys = tuple(np.array(x, copy=True) for x in ba.reduced_system(dense=False))
    return out


_envelope_cache = {}


def _envelope(gpu, c, key=(), **kw):
    """The envelope Cholesky's pass of the case (once per case and setting)."""
    k = (c.name, c.na, key)
    if k not in _envelope_cache:
        _envelope_cache[k] = _pass(gpu, c, "envelope", **kw)
    return _envelope_cache[k]


def _check_stop_rule(p, tol, max_iter=2000):
    true = pcg_ref.true_relres(*p.sys, p.da)
    print(f"  tol {tol:g}: {p.stats['iterations']} iterations, relres {p.stats['relres']:.4g}, "
          f"true {true:.4g}")
    assert p.pinv == 0 and p.stats["converged"], p.stats
    assert 1 <= p.stats["iterations"] < max_iter and p.stats["relres"] <= tol, p.stats
    assert true <= 1.01 * tol, (true, tol)


_ref_cache = {}


def _direct_bound(p, key):
    """(10 x the distance of pcg_ref's solution at tolerance 1e-12 from the
    long double direct solve of the same downloaded blocks, floor 1e-12; the
    pass's own distance from that direct solve)."""
    if key not in _ref_cache:
        x = pcg_ref.direct(*p.sys)
        ref = pcg_ref.pcg(*p.sys, 1e-12, 2000)
        assert ref["status"] == 0 and ref["converged"], ref
        scale = float(np.abs(x).max())
        _ref_cache[key] = (x, float(np.abs(ref["da"] - x).max()) / scale)
    x, ref_err = _ref_cache[key]
    own = float(np.abs(p.da.reshape(-1, order="F") - x).max() / np.abs(x).max())
    return max(10.0 * ref_err, 1e-12), own


def _rel(da, da_env, rows=None):
    d, e = da.reshape(-1, order="F"), da_env.reshape(-1, order="F")
    if rows is not None:
        d, e = d[rows], e[rows]
    return float(np.abs(d - e).max() / np.abs(e).max())


CASES = [("ladybug40", 6), ("ladybug120", 6), ("cfg2", 7), ("shared", 6), ("cfg2", 9),
         ("cfg2", 10), ("cfg2", 12), ("m2", 6), ("m1", 6)]


# ---- 1. the stop rule ------------------------------------------------------------
@pytest.mark.parametrize("name,na", CASES)
def test_stop_rule_honoured(gpu, name, na):
    c = _case(name, na)
    env = _envelope(gpu, c)
    print(f"PCG {name} num_a {na}:")
    for tol in (1e-2, 1e-6, 1e-8):
        p = _pass(gpu, c, "pcg", tol, 2000)
        _check_stop_rule(p, tol)
        assert p.old == env.old                   # the same linearisation, bit for bit
        assert p.plan["pcg"] == 1 and p.plan["ordered"] == 0


# ---- 2. against the direct solve -------------------------------------------------
@pytest.mark.parametrize("name,na", [("ladybug40", 6), ("ladybug120", 6), ("cfg2", 7),
                                     ("shared", 6), ("m2", 6)])
def test_agrees_with_the_direct_solve(gpu, name, na):
    c = _case(name, na)
    env = _envelope(gpu, c)
    p = _pass(gpu, c, "pcg", 1e-12, 2000)
    bound, own = _direct_bound(p, (name, na))
    got = _rel(p.da, env.da)
    print(f"PCG-DIRECT {name} num_a {na}: {p.stats['iterations']} iterations, |da - da_env| "
          f"{got:.3g} of max |da_env|, bound {bound:.3g}; from the long double solve: pcg "
          f"{own:.3g}, envelope {_rel(env.da, np.asarray(_ref_cache[(name, na)][0], dtype=float)):.3g}")
    assert p.stats["converged"] and p.pinv == 0
    assert got <= bound, (got, bound)


# ---- 3. exactly-zero rows --------------------------------------------------------
def _zero_case(kind):
    """(case, context keywords, start a, the rows that must be exactly zero)."""
    if kind == "noobs":
        c = _case("noobs", 6)
        return c, {}, c.a, np.arange(6 * 7, 6 * 8)
    c = _case("ladybug40", 6)
    ld = 6 * c.m
    if kind == "pivot":
        return c, dict(pivot=np.arange(c.m) < 2), c.a, np.arange(12)
    if kind == "fix_motion":
        return c, dict(fix_motion=True), c.a, np.arange(ld)
    if kind == "w0":        # forward differences leave the rotation columns of w = 0 zero
        a = c.a.copy(order="F")
        a[0:3, 5] = 0.0
        return c, dict(jacobian="fd"), a, np.arange(6 * 5, 6 * 5 + 3)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["pivot", "fix_motion", "noobs", "w0"])
def test_zero_rows(gpu, kind):
    c, kw, a, rows = _zero_case(kind)
    env = _envelope(gpu, c, key=kind, a=a, **kw)
    p = _pass(gpu, c, "pcg", 1e-12, 2000, a=a, **kw)
    da = p.da.reshape(-1, order="F")
    assert np.array_equal(da[rows], np.zeros(len(rows)))
    assert np.array_equal(env.da.reshape(-1, order="F")[rows], np.zeros(len(rows)))
    assert p.pinv == 0 and p.old == env.old
    other = np.setdiff1d(np.arange(da.size), rows)
    if kind == "fix_motion":    # every row is zero: nothing to iterate on
        assert other.size == 0 and p.stats["iterations"] == 0 and p.stats["converged"]
        return
    assert p.stats["converged"] and p.stats["iterations"] >= 1
    bound, _ = _direct_bound(p, ("zero", kind))
    got = _rel(p.da, env.da, other)
    print(f"PCG-ZERO {kind}: {p.stats['iterations']} iterations, other rows {got:.3g}, "
          f"bound {bound:.3g}")
    assert got <= bound, (got, bound)


# ---- 4. determinism, the iteration limit, m = 1 ---------------------------------
def test_same_bits_twice(gpu):
    c = _case("shared", 6)
    with _make(gpu, c, "pcg", pcg_tol=1e-8, pcg_max_iter=2000) as ba:
        ba.set_params(c.a, c.b)
        out = []
        for _ in range(2):
            i = ba.step(relinearize=True, update_lm=False)
            out.append((ba.last_step()[0].copy(), ba.pcg_stats(), i.new_sse, i.dpg))
        assert out[0][1]["total"] == out[0][1]["iterations"]
        assert out[1][1]["total"] == 2 * out[0][1]["iterations"]
    q = _pass(gpu, c, "pcg", 1e-8, 2000)      # ... and a second context
    for da, st, new, dpg in (out[1], (q.da, q.stats, q.new, q.dpg)):
        assert np.array_equal(da, out[0][0])
        assert (st["iterations"], st["relres"]) == (out[0][1]["iterations"], out[0][1]["relres"])
        assert (new, dpg) == out[0][2:]


@pytest.mark.parametrize("limit", [3, 8, 9, 25])
def test_iteration_limit_ends_the_solve(gpu, limit):
    """3: inside the first batch of launches; 8 / 9: its last iteration and
    the first of the second batch; 25: inside the third."""
    c = _case("ladybug40", 6)
    env = _envelope(gpu, c)
    p = _pass(gpu, c, "pcg", 1e-12, limit)
    assert p.stats["iterations"] == limit and not p.stats["converged"], p.stats
    assert p.stats["relres"] > 1e-12 and p.pinv == 0
    assert np.all(np.isfinite(p.da)) and p.dpg > 0 and np.isfinite(p.new)
    assert p.acc == int(p.old - p.new > 0)            # the ordinary rule, no error
    assert p.old == env.old
    # the recurrence's residual is the iterate's true one (1 %, as in test 1)
    true = pcg_ref.true_relres(*p.sys, p.da)
    assert abs(true - p.stats["relres"]) <= 0.01 * true, (true, p.stats)


def test_one_camera_converges_in_one_iteration(gpu):
    p = _pass(gpu, _case("m1", 6), "pcg", 1e-6, 2000)
    assert p.stats["iterations"] == 1 and p.stats["converged"], p.stats


# ---- 5. the fallback ---------------------------------------------------------------
def test_forced_pivot_takes_the_pinv_step(gpu):
    c = _case("ladybug40", 6)
    force = lambda ba: ba.force_status(4, 1)   # noqa: E731
    env = _pass(gpu, c, "envelope", prepare=force)
    p = _pass(gpu, c, "pcg", 1e-6, 2000, prepare=force)
    assert p.pinv == 1 and env.pinv == 1
    assert p.old == env.old and p.acc == env.acc
    assert abs(p.new - env.new) <= 1e-9 * env.new
    # a forced word 5 solves again the same way
    q = _pass(gpu, c, "pcg", 1e-6, 2000, prepare=lambda ba: ba.force_status(5, 1))
    r = _pass(gpu, c, "pcg", 1e-6, 2000)
    assert q.pinv == 0 and np.array_equal(q.da, r.da) and q.new == r.new
    assert q.stats["total"] == 2 * r.stats["total"]


# ---- 6. whole runs ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(gpu, solver, tol):
    c = _case("ladybug120", 6)
    kw = dict(pcg_tol=tol, pcg_max_iter=2000) if solver == "pcg" else {}
    with _make(gpu, c, solver, stop_rel=1e-9, max_iter=15, **kw) as ba:
        ba.set_params(c.a, c.b)
        err, st = ba.run()
        return err.copy(), st.iterations, (ba.pcg_stats()["total"] if solver == "pcg" else 0)


def test_whole_run_tight_tolerance_follows_the_direct_run(gpu):
    e0, n0, _ = _run(gpu, "envelope", None)
    e1, n1, total = _run(gpu, "pcg", 1e-10)
    n = min(len(e0), len(e1))
    print(f"PCG-RUN tol 1e-10: {n1} passes ({n0} direct), {total} CG iterations, error_ "
          f"differences {np.abs(e1[:n] - e0[:n]) / e0[:n]}")
    assert n >= 3
    assert np.allclose(e1[:n], e0[:n], rtol=1e-6, atol=0), (e1[:n] - e0[:n]) / e0[:n]


def test_whole_run_default_tolerance_ends_at_the_same_cost(gpu):
    e0, n0, _ = _run(gpu, "envelope", None)
    e1, n1, total = _run(gpu, "pcg", 0.1)
    print(f"PCG-RUN tol 0.1: {n1} passes ({n0} direct), {total} CG iterations, final error_ "
          f"{e1[-1]:.12g} vs {e0[-1]:.12g}")
    assert abs(e1[-1] - e0[-1]) <= 1e-6 * e0[-1], (e1, e0)


# ---- 7. memory and plan -------------------------------------------------------------
@pytest.mark.parametrize("name,na", [("ladybug120", 6), ("cfg2", 10), ("m1", 6)])
def test_memory_and_plan(gpu, name, na):
    c = _case(name, na)
    with _make(gpu, c, "pcg") as ba:
        p = ba.plan_info()
        assert ba.get_pcg() == (0.1, 500)
    m, nb, ld = p["cameras"], p["blocks"], p["num_a"] * p["cameras"]
    assert (m, p["num_a"]) == (c.m, na)
    assert p["pcg"] == 1
    assert p["solve_bytes"] == (8 * (4 + na) * ld + ld + 16 * ((m + 3) // 4) + 64 + 8 * m + 4
                                + 24 * nb)
    assert p["cr_levels"] == 0 and p["tiles"] == 0
    assert all(p[k] == 0 for k in ("cr_elim", "cr_keep", "cr_rows", "nd_arcs", "nd_sep_tiles",
                                   "solve_flops_factor", "solve_flops_syrk", "solve_flops_back",
                                   "env_runner_runs", "camupd_fold"))
    with _make(gpu, c, "envelope") as ba:
        e = ba.plan_info()
    lds = 64 * ((ld + 63) // 64)
    assert e["pcg"] == 0 and e["solve_bytes"] >= 8 * lds * lds
    assert all(e[k] == p[k] for k in ("obs", "points", "cameras", "blocks", "chunks", "groups"))


def test_settings(gpu):
    from bundleadjustmentmatlab_amd._lib import VlgbaError
    c = _case("m2", 6)
    with _make(gpu, c, "pcg", pcg_tol=1e-3) as ba:
        assert ba.get_pcg() == (1e-3, 500)
        ba.set_pcg(max_iter=7)
        assert ba.get_pcg() == (1e-3, 7)
        ba.set_pcg(0.5)
        assert ba.get_pcg() == (0.5, 7)
        for bad in (1.0, 2.0, float("nan"), float("inf")):
            with pytest.raises(VlgbaError, match="-1001"):
                ba.set_pcg(bad)
        assert ba.get_pcg() == (0.5, 7)
        assert ba.pcg_stats() == dict(iterations=0, relres=0.0, converged=False, total=0)
    with _make(gpu, c, "envelope") as ba:
        for call in (ba.get_pcg, ba.pcg_stats, lambda: ba.set_pcg(0.1)):
            with pytest.raises(VlgbaError, match="-1001"):
                call()


# ---- 8. refusals and neighbours -------------------------------------------------------
def test_refusals(gpu):
    from bundleadjustmentmatlab_amd._lib import VlgbaError
    c = _case("ladybug40", 6)
    for kw in (dict(parity=True), dict(ordered=True)):
        with pytest.raises(VlgbaError, match="-1001"):
            _make(gpu, c, "pcg", **kw)
    with _make(gpu, c, "pcg") as ba:
        with pytest.raises(VlgbaError, match="-1001"):
            ba.set_covariance_method("selected")
        assert ba.get_covariance_method() == "dense"


def test_dense_covariance_is_the_envelope_contexts(gpu):
    c = _case("ladybug40", 6)
    out = {}
    for solver in ("envelope", "pcg"):
        with _make(gpu, c, solver, pivot=np.arange(c.m) < 2) as ba:
            ba.set_params(c.a, c.b)
            out[solver] = ba.covariance()
    for k in ("cam", "pts"):
        assert np.array_equal(out["pcg"][k], out["envelope"][k]), k
    assert out["pcg"]["sigma2"] == out["envelope"]["sigma2"]


@pytest.mark.parametrize("kw", [dict(loss="huber", loss_scale=2.0), dict(jacobian="analytic")],
                         ids=["huber", "analytic"])
def test_composes_with_loss_and_analytic_jacobians(gpu, kw):
    c = _case("ladybug40", 6)
    env = _envelope(gpu, c, key=tuple(kw), **kw)
    p = _pass(gpu, c, "pcg", 1e-6, 2000, **kw)
    print(f"PCG {tuple(kw)}:")
    _check_stop_rule(p, 1e-6)
    assert p.old == env.old
