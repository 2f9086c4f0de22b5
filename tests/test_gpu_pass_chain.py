"""The LM pass's chain of small launches ("the pass chain"):

  * V*^-1 inside the MFMA Schur launch (ba_dev::vinv_fold, VLGBA_VINV_FOLD):
    each Schur group's workgroup forms the damped vlg_pinv3 of its own points
    in its prologue instead of a k_point_vinv launch over all points (timed as
    k_damp_point) -- allowed only when the MFMA groups' point ranges tile
    every point;
  * the camera update inside the one-launch cyclic reduction
    (ba_dev::camupd_fold, VLGBA_CAMUPD_FOLD): a back record forms a_new = a +
    da and the rotation table of its own cameras, the update's final sums form
    the camera part of dp'(lambda dp + g), and the update that directly
    follows that solve launches no k_camera_update -- every other solve's
    (the no-spin re-solve, the pinv step) does.

Each case compares the fold on against the fold off (the launch it replaces),
from the same start, bit for bit: four applied passes (scalars and steps), one
relinearising pass, a whole run (error_ and parameters).  a_new and the
rotation tables are compared through what depends on them: the fused update
linearises at them, so the next passes' scalars and steps carry them; once
more with VLGBA_FUSED=0, where the separate update kernel reads them.  With
the pass timers on, the folded context shows no launch of the replaced kernel
in a pass and the other context one.

The thinned scene puts points no camera sees (V = 0: the zero block) and points
seen once (rank-deficient V) inside the Schur groups' ranges; the posterior
covariance's undamped Schur phase (lambda = 0) then takes vlg_pinv3's Jacobi
branch for the latter inside the Schur launch.

The last section holds what one launch of a pass leaves for another (the
camera reduction to fold, the side stream's join, the publish) to the three
plan kinds that route them differently: against the other entry points run
between passes, timed against untimed passes, and -- stage 1 being one
function for the pass, the getters and the covariance -- parity mode's
sequential old SSE after a getter.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = {"vinv": ("VLGBA_VINV_FOLD", "vinv_fold", "k_damp_point"),
          "camupd": ("VLGBA_CAMUPD_FOLD", "camupd_fold", "k_camera_update")}


def _banded(m=30, n=3000, track=6, seed=17):
    from bundleadjustmentmatlab_amd.scene import banded_scene
    return banded_scene(m=m, n=n, track=track, seed=seed)


def _thinned():
    """The banded scene with every 97th point unseen and every 50th seen once."""
    import dataclasses
    sc = _banded()
    first = np.r_[True, sc.obs_pt[1:] != sc.obs_pt[:-1]]       # point-major order
    keep = np.ones(sc.obs_pt.size, dtype=bool)
    keep[(sc.obs_pt % 50 == 0) & ~first] = False
    keep[sc.obs_pt % 97 == 0] = False
    return dataclasses.replace(sc, obs_pt=sc.obs_pt[keep], obs_cam=sc.obs_cam[keep],
                               obs_x=sc.obs_x[keep])


def _long():
    from bundleadjustmentmatlab_amd.scene import make_config
    return make_config("ladybug", m=300, n=5000, max_track=30, radius=150.0, seed=29,
                       long_frac=0.01, long_len=(100, 220))


def _make(gpu, sc, num_a, kw, env):
    """A context created with the environment switches of env ({name: "0"})."""
    kw = dict(kw)
    if kw.get("pivot") == "first2":
        kw["pivot"] = np.arange(sc.m) < 2
    names = ("VLGBA_VINV_FOLD", "VLGBA_CAMUPD_FOLD", "VLGBA_FUSED")
    old = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(env)
    try:
        return gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, num_a, **kw)
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _start(sc, num_a):
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    return a, np.asfortranarray(sc.X0[:3])


def _info(i):
    return (i.old_sse, i.new_sse, i.dpg, i.accepted, i.lambda_, i.pinv)


def _launches(ba, kernel, force=None):
    """Launches of `kernel` in one timed pass (after force_status(*force))."""
    ba.set_timing(True)
    ba.kernel_ms(reset=True)
    if force:
        ba.force_status(*force)
    i = ba.step(relinearize=True, update_lm=False)
    k = ba.kernel_ms(reset=True)
    ba.set_timing(False)
    return k.get(kernel, (0.0, 0))[1], i


def _trajectory(gpu, sc, num_a, kw, env, part, whole_run=True):
    ba = _make(gpu, sc, num_a, kw, env)
    plan = ba.plan_info()
    a, b = _start(sc, num_a)
    ba.set_params(a, b)
    steps = []
    for _ in range(4):
        i = ba.step(relinearize=False, update_lm=True)
        da, db = ba.last_step()
        steps.append((_info(i), da.copy(), db.copy()))
    launches, i = _launches(ba, SWITCH[part][2])
    da, db = ba.last_step()
    steps.append((_info(i), da.copy(), db.copy()))
    err, params = None, None
    if whole_run:
        ba.set_params(a, b)
        err, _ = ba.run()
        params = ba.get_params()
    ba.close()
    return dict(plan=plan, steps=steps, launches=launches, err=err, params=params)


def _same(r1, r0, what):
    for k, (u, v) in enumerate(zip(r1["steps"], r0["steps"])):
        assert u[0] == v[0], (what, k, u[0], v[0])
        assert np.array_equal(u[1], v[1]) and np.array_equal(u[2], v[2]), (what, k)
    if r1["err"] is not None:
        assert np.array_equal(r1["err"], r0["err"]), (what, r1["err"], r0["err"])
        assert all(np.array_equal(x, y) for x, y in zip(r1["params"], r0["params"])), what


def _on_off(gpu, sc, num_a, kw, part, expect_on=True, extra_env=None):
    var, key, _ = SWITCH[part]
    env = dict(extra_env or {})
    on = _trajectory(gpu, sc, num_a, kw, env, part)
    off = _trajectory(gpu, sc, num_a, kw, dict(env, **{var: "0"}), part)
    assert off["plan"][key] == 0 and off["launches"] == 1, (off["plan"][key], off["launches"])
    assert on["plan"][key] == int(expect_on), on["plan"]
    assert on["launches"] == (0 if expect_on else 1), on["launches"]
    _same(on, off, (part, kw))
    return on, off


# ---- V*^-1 inside the MFMA Schur launch -----------------------------------
VINV_CASES = [("plain", {}), ("fixstruct", dict(fix_structure=True)),
              ("pivot", dict(pivot="first2"))]


@pytest.mark.parametrize("kind,kw", VINV_CASES)
def test_vinv_fold_bit_identical(gpu, kind, kw):
    on, _ = _on_off(gpu, _banded(), 6, kw, "vinv")
    assert on["plan"]["mfma_groups"] == on["plan"]["groups"] > 1, on["plan"]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_vinv_fold_bit_identical_at_the_batch_edge(gpu, n):
    """k_point_vinv's 256-point batches (the fold off) against the Schur
    groups' prologues (the fold on), which run the same routine over their own
    few points: a partial batch, exactly one batch, one batch and one point."""
    on, _ = _on_off(gpu, _banded(m=30, n=n), 6, {}, "vinv")
    assert on["plan"]["mfma_groups"] == on["plan"]["groups"] > 1, on["plan"]


def test_vinv_fold_separate_update_kernels(gpu):
    """VLGBA_FUSED=0: k_point_update_chunk reads the folded V*^-1."""
    _on_off(gpu, _banded(), 6, {}, "vinv", extra_env={"VLGBA_FUSED": "0"})


def test_vinv_fold_unseen_and_rank_deficient_points(gpu):
    sc = _thinned()
    cnt = np.bincount(sc.obs_pt, minlength=sc.n)
    assert sc.n == 3000 and (cnt == 0).sum() == 31 and (cnt == 1).sum() == 59, (
        (cnt == 0).sum(), (cnt == 1).sum())
    on, off = _on_off(gpu, sc, 6, {}, "vinv")
    # a point no camera sees gets the zero block: its db is exactly zero
    for r in (on, off):
        assert np.all(r["steps"][0][2][:, cnt == 0] == 0.0)
    # lambda = 0 (the covariance's undamped Schur phase): V of a point seen
    # once is singular, vlg_pinv3 takes its Jacobi branch inside the launch
    cov = {}
    for fold in (True, False):
        ba = _make(gpu, sc, 6, dict(pivot="first2"), {} if fold else {"VLGBA_VINV_FOLD": "0"})
        assert ba.plan_info()["vinv_fold"] == int(fold)
        ba.set_params(*_start(sc, 6))
        c = ba.covariance(scale=False)
        cov[fold] = (c["cam"].copy(), c["pts"].copy())
        ba.close()
    assert np.array_equal(cov[True][0], cov[False][0])
    assert np.array_equal(cov[True][1], cov[False][1])
    assert np.all(np.isfinite(cov[True][1]))


def test_vinv_fold_off_on_mixed_plan(gpu):
    """Per-term groups and long tracks beside the MFMA groups: their points get
    V*^-1 from k_point_vinv, so the fold stays off and the switch changes
    nothing."""
    sc = _long()
    res = []
    for env in ({}, {"VLGBA_VINV_FOLD": "0"}):
        r = _trajectory(gpu, sc, 6, {}, env, "vinv", whole_run=False)
        assert r["plan"]["vinv_fold"] == 0 and r["plan"]["long_points"] > 0, r["plan"]
        assert r["launches"] >= 1, r["launches"]
        res.append(r)
    _same(res[0], res[1], "long")


# ---- the camera update inside the one-launch cyclic reduction --------------
@pytest.mark.parametrize("m", [30, 32, 33])
@pytest.mark.parametrize("num_a", [6, 7, 10])
def test_camupd_fold_bit_identical(gpu, num_a, m):
    """m = 30: whole tiles for num_a 6 and 10 (30 rows), m = 32: for num_a 7 (28
    rows); the others leave a partial last tile.  The camera-aligned tiles need
    every track inside two neighbouring groups of floor(32 / num_a) cameras:
    tracks of 6 views for num_a 6 (5 cameras a tile), of 4 for num_a 7 and 10
    (4 and 3 cameras a tile)."""
    on, _ = _on_off(gpu, _banded(m=m, track=6 if num_a == 6 else 4), num_a, {}, "camupd")
    assert on["plan"]["cr_levels"] > 0 and on["plan"]["cr_rows"] == num_a * (32 // num_a)


@pytest.mark.parametrize("kind,kw", [("fixmotion", dict(fix_motion=True)),
                                     ("pivot", dict(pivot="first2"))])
def test_camupd_fold_fix_masks(gpu, kind, kw):
    _on_off(gpu, _banded(m=33), 6, kw, "camupd")


def test_camupd_fold_separate_update_kernels(gpu):
    """VLGBA_FUSED=0: k_point_update_chunk reads a_new and rot_new."""
    _on_off(gpu, _banded(m=33), 6, {}, "camupd", extra_env={"VLGBA_FUSED": "0"})


@pytest.mark.parametrize("word,field", [(5, "spin_retry"), (4, "pinv")])
def test_camupd_fold_fallback_solves_launch_the_update(gpu, word, field):
    """force_status(5, 1): the pass re-solves without spins (per-level launches);
    force_status(4, 1): it takes the pinv step.  Either da is not the one-launch
    CR's, so the update after it launches k_camera_update itself -- single step
    and whole run, fold on against off, bit for bit."""
    sc = _banded(m=33)
    a, b = _start(sc, 6)
    res = {}
    for fold in (True, False):
        ba = _make(gpu, sc, 6, {}, {} if fold else {"VLGBA_CAMUPD_FOLD": "0"})
        assert ba.plan_info()["camupd_fold"] == int(fold)
        ba.set_params(a, b)
        ba.force_status(word, 1)
        i = ba.step(relinearize=False, update_lm=True)
        da, db = ba.last_step()
        step = (_info(i), getattr(i, field), da.copy(), db.copy())
        j = ba.step(relinearize=False, update_lm=True)       # the hook is spent
        nxt = (_info(j), getattr(j, field))
        launches, k = _launches(ba, "k_camera_update", force=(word, 1))
        assert getattr(k, field) == 1
        ba.set_params(a, b)
        ba.force_status(word, 1)
        err, st = ba.run()
        res[fold] = (step, nxt, launches, err, ba.get_params())
        ba.close()
    r1, r0 = res[True], res[False]
    assert r1[0][1] == 1 and r1[1][1] == 0, (r1[0][:2], r1[1])
    # the first update of the forced pass is the folded one (no launch), the
    # fallback's is not; without the fold both launch
    assert (r1[2], r0[2]) == (1, 2), (r1[2], r0[2])
    assert r1[0][:2] == r0[0][:2] and r1[1] == r0[1], (r1[0][:2], r0[0][:2])
    assert np.array_equal(r1[0][2], r0[0][2]) and np.array_equal(r1[0][3], r0[0][3])
    assert np.array_equal(r1[3], r0[3]), (r1[3], r0[3])
    assert all(np.array_equal(x, y) for x, y in zip(r1[4], r0[4]))


def test_camupd_fold_across_entry_points(gpu):
    """Whether a solve did the camera update is handed from that solve to the
    update of the same pass and lives nowhere else, so solver code that runs
    between passes cannot leave it behind: two steps, then the selected-inverse
    covariance (the per-level factor launches alone, no back substitution, no
    update), get_step and get_reduced_system, then two more steps -- fold on
    against off, bit for bit.  The first two cameras are the pivot (the gauge
    is fixed, as in test_camupd_fold_fix_masks), so the covariance succeeds and
    is compared too."""
    sc = _banded(m=33)
    a, b = _start(sc, 6)
    res = {}
    for fold in (True, False):
        ba = _make(gpu, sc, 6, dict(pivot="first2"),
                   {} if fold else {"VLGBA_CAMUPD_FOLD": "0"})
        assert ba.plan_info()["camupd_fold"] == int(fold)
        ba.set_params(a, b)
        sse = []
        for _ in range(2):
            i = ba.step(relinearize=False, update_lm=True)
            sse.append((i.old_sse, i.new_sse))
        cov = ba.covariance(scale=False, method="selected")
        cov = (cov["cam"], cov["pts"])
        da, db = ba.last_step()
        jk, blocks, e_ = ba.reduced_system(dense=False)
        for _ in range(2):
            i = ba.step(relinearize=False, update_lm=True)
            sse.append((i.old_sse, i.new_sse))
        params = ba.get_params()
        launches, _ = _launches(ba, "k_camera_update")
        res[fold] = dict(sse=sse, cov=cov, step=(da, db), red=(blocks, e_), params=params,
                         launches=launches)
        ba.close()
    r1, r0 = res[True], res[False]
    print(f"CAMUPD entry points: sse {r1['sse']} | {r0['sse']}; k_camera_update launches "
          f"{r1['launches']} | {r0['launches']}")
    assert (r1["launches"], r0["launches"]) == (0, 1)
    assert r1["sse"] == r0["sse"], (r1["sse"], r0["sse"])
    assert all(np.array_equal(x, y) for x, y in zip(r1["params"], r0["params"]))
    assert all(np.array_equal(x, y) for x, y in zip(r1["step"], r0["step"]))
    assert all(np.array_equal(x, y) for x, y in zip(r1["red"], r0["red"]))
    assert all(np.isfinite(x).all() for x in r1["cov"])
    assert all(np.array_equal(x, y) for x, y in zip(r1["cov"], r0["cov"]))


# ---- what one launch of a pass leaves for another --------------------------
# The three ways a pass routes its camera reduction and Schur launches
# (plan_info): every group an MFMA group (the reduction's workgroups and the
# publish ride on the pass's own launches), the per-term kernel alone (the
# reduction on the side stream, joined before k_schur_reduce), both kinds (the
# per-term groups on the side stream beside the MFMA groups).
PLAN_KINDS = ("mfma", "term", "mixed")


def _plan_kind_ctx(gpu, kind, sc=None):
    sc = sc or (_long() if kind == "mixed" else _banded())
    kw = dict(pivot="first2")              # the gauge fixed: the covariance exists
    if kind == "term":
        kw["schur_kernel"] = "terms"
    ba = _make(gpu, sc, 6, kw, {})
    p = ba.plan_info()
    assert p["ordered"] == 0 and p["groups"] > 1, p
    if kind == "mfma":
        assert p["mfma_groups"] == p["groups"], p
    elif kind == "term":
        assert p["mfma_groups"] == 0 and p["mfma"] == 0, p
    else:
        assert 0 < p["mfma_groups"] < p["groups"], p
    ba.set_params(*_start(sc, 6))
    return ba


def _pass_record(ba, relinearize):
    i = ba.step(relinearize=relinearize, update_lm=True)
    da, db = ba.last_step()
    return (i.old_sse, i.new_sse, i.dpg, i.accepted, i.lambda_), da.copy(), db.copy()


def _same_passes(ra, rb, what):
    assert len(ra) == len(rb)
    for k, (u, v) in enumerate(zip(ra, rb)):
        assert u[0] == v[0], (what, k, u[0], v[0])
        assert np.array_equal(u[1], v[1]) and np.array_equal(u[2], v[2]), (what, k)


@pytest.mark.parametrize("kind", PLAN_KINDS)
def test_handoffs_survive_the_entry_points_between_passes(gpu, kind):
    """The camera reduction to fold, the side stream's join and the publish
    are arguments and locals of one pass, so nothing another entry point
    launches between two passes can leave one of them behind or consume it:
    four applied passes and a relinearising one, alone and with
    get_linearization, get_reduced_system, the dense covariance (an undamped
    Schur phase on the same buffers) and get_step between every two of them
    -- scalars, steps and final parameters bit for bit."""
    res = {}
    for between in (False, True):
        ba = _plan_kind_ctx(gpu, kind)
        recs = []
        for k in range(5):
            recs.append(_pass_record(ba, relinearize=(k == 4)))
            if between and k < 4:
                lin = ba.linearization()
                S, e_ = ba.reduced_system(dense=False)[1:]
                cov = ba.covariance(scale=False, method="dense")
                da, db = ba.last_step()
                assert np.array_equal(da, recs[-1][1]) and np.array_equal(db, recs[-1][2])
                assert all(np.isfinite(x).all() for x in
                           (lin["U"], lin["eA"], S, e_, cov["cam"], cov["pts"]))
        res[between] = (recs, ba.get_params())
        ba.close()
    print(f"HANDOFFS {kind}: " + "; ".join(repr(r[0]) for r in res[True][0]))
    _same_passes(res[True][0], res[False][0], kind)
    assert all(np.array_equal(x, y) for x, y in zip(res[True][1], res[False][1])), kind


@pytest.mark.parametrize("kind", PLAN_KINDS)
def test_timed_and_untimed_passes_agree(gpu, kind):
    """A timed pass launches nothing on the side stream, copies its scalars
    instead of spinning on them and publishes nothing from the update's final
    sums; the kernels and their inputs are the untimed pass's, so four
    applied passes give the same scalars, steps and parameters bit for bit."""
    res = {}
    for timed in (False, True):
        ba = _plan_kind_ctx(gpu, kind)
        ba.set_timing(timed)
        recs = [_pass_record(ba, relinearize=False) for _ in range(4)]
        res[timed] = (recs, ba.get_params())
        ba.close()
    print(f"TIMED {kind}: " + "; ".join(repr(r[0]) for r in res[True][0]))
    _same_passes(res[True][0], res[False][0], kind)
    assert all(np.array_equal(x, y) for x, y in zip(res[True][1], res[False][1])), kind


@pytest.mark.parametrize("getter", ["reduced_system", "linearization"])
def test_parity_old_sse_after_a_getter(gpu, getter):
    """Parity mode sums the old SSE sequentially in the reference's flat order
    (k_seq_old_sse) wherever stage 1 runs.  A getter that runs stage 1 after
    set_params marks the linearisation valid, so the step after it
    (relinearize=False) runs no stage 1 of its own and reports the getter's old
    SSE: the same digits as a step that runs stage 1 itself.

    The library before the shared stage 1 left the getters' old SSE to
    k_sum_parts' order; the figures of both libraries on this scene are in
    profiles/pass_handoffs/README.md."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg1", m=6, min_n=30, max_n=60, seed=7)   # test_gpu_lm_parity's "small"
    assert sc.n < 200
    a, b = _start(sc, 6)
    res = {}
    for first in (getter, None):
        ba = gpu.BundleAdjuster(sc.K, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.n, 6, parity=True)
        assert ba.plan_info()["ordered"] == 1
        ba.set_params(a, b)
        if first:
            getattr(ba, first)()
        i = ba.step(relinearize=False, update_lm=False)
        res[first] = (repr(i.old_sse), repr(i.new_sse), repr(i.dpg))
        ba.close()
    print(f"PARITY old SSE after {getter}: {res[getter]} | alone {res[None]}")
    assert res[getter] == res[None], (res[getter], res[None])
