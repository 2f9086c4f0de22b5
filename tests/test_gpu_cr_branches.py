"""Both cyclic reductions on every branch they choose by the device's
compute-unit count, entry by entry against the solve reference: the
componentwise backward error eta of da in the GPU's own S da = e_, in long
double, at most ld * u -- tests/test_gpu_stage_ref.py::test_solve_stage's bar,
unchanged -- from the getter's blocks (schur_ref.residual_blocks, proven on the
CPU by tests/test_schur_ref.py; the dense S of the large cases would be over a
gigabyte).

The scenes and the branch predicates are tests/cr_branches.py's; their routes
are proven without a GPU by tests/test_cr_branch_kinds.py.  Here the same
predicates run with the device's real compute-unit count, and the launch counts
of one timed pass pin the route: k_cr_factor and k_cr_back once a level,
k_cr_update once a level with a kept tile, no k_factor_step; cr_rows == 64
(ba_solver.cpp vlgba_plan_info: the 64-row route reports its tile height).

A. the 64-row reduction (k_cr_factor / k_cr_update / k_cr_back), num_a 6 / 7 / 9
   / 10 / 12: two to ten tiles with partial, full and straddled last tiles
   (split bodies), and 110 / 132 tiles, where level 0 runs the UNSPLIT body of
   k_cr_factor (all three) and of k_cr_update (the two of 132 tiles) and every
   deeper level the split ones.  Small cases: both residuals (they agree within
   schur_ref.residual_slack) and LAPACK's dense Cholesky beside the GPU; large
   cases: the blockwise residual alone, LAPACK's banded Cholesky (dpbsv) on the
   same S beside it -- the dense figure is left out.
B. masks: two pivot cameras, and a camera without observations in the middle
   (unit diagonal from k_assemble_tiles): da exactly 0 there, eta over the rest.
C. no state carried between solves (the reduction overwrites S's diagonal
   tiles, leaves fill tiles outside the envelope and keeps linv / crL / ywork):
   two solves of one linearisation are bit-identical in da and db, and a third
   after an applied LM step meets the bar against the new S.
D. the camera-aligned 32-row reduction at 600 tiles (m = 3000), one launch and
   level by level: level 0 in two records a tile, k_cr32_factor unsplit, the
   back substitution one launch a level.

Every test prints its figures before it asserts (lines starting CR-BRANCH,
pytest -s).  A device on which the large cases do not reach these branches
fails the test; it does not skip.

Measured on an MI355X (256 compute units); no bar was widened, the worst solve
is 0.081 of it.  eta / (ld u), GPU | LAPACK Cholesky on the same S (dense for
the small cases, banded dpbsv for the large ones); the kinds are factor then
update per level, s split, u unsplit, - no launch:
    scene (ld, tiles)                 kinds                       GPU     | LAPACK
    num_a  6, track  9, m 11 (66, 2)     ss s-                    0.081   | 0.025
    num_a  6, track  9, m 22 (132, 3)    ss s-                    0.068   | 0.013
    num_a  6, track  9, m 43 (258, 5)    ss ss s-                 0.030   | 0.0087
    num_a  6, track  9, m 64 (384, 6)    ss ss s-                 0.014   | 0.0053
    num_a  6, track 10, m 43 (258, 5)    ss ss s-                 0.057   | 0.0073
    num_a  7, track  8, m 75 (525, 9)    ss ss ss s-              0.0058  | 0.0043
    num_a  9, track  6, m 33 (297, 5)    ss ss s-                 0.013   | 0.0050
    num_a 10, track  6, m 64 (640, 10)   ss ss ss s-              0.0055  | 0.0030
    num_a 12, track  5, m 33 (396, 7)    ss ss s-                 0.0074  | 0.0042
    num_a 10, track  5, m 700 (7000, 110)  us ss ss ss ss ss s-   0.0021  | 0.00048
    num_a 12, track  5, m 700 (8400, 132)  uu ss ss ss ss ss ss s-  0.00045 | 0.00050
    num_a  6, track  9, m 1400 (8400, 132) uu ss ss ss ss ss ss s-  0.0046  | 0.00058
    two pivot cameras, num_a 6, m 43     ss ss s-                 0.030   | 0.0076
    camera 31 unseen, num_a 10, m 64     ss ss ss s-              0.0046  | 0.0027
    32-row, num_a 6, m 3000 (18000, 600 tiles, 10 levels), one launch and per
    level: 0.00073 | 0.00022, da and db bit-identical between the two
The projective num_a 12, m 700 scene keeps lambda 1e-3: the GPU's and LAPACK's
Cholesky of its S both succeed there (no non-positive pivot).  The blockwise
and the dense residual agree to the digits printed on every small case.
Repeated solves: bit-identical da and db at m 75 (num_a 7) and m 1400 (num_a 6);
the third solve after the applied step (lambda 1e-3 -> 3.3e-4) 0.0052 / 0.0014.
"""
import numpy as np
import pytest

import cr_branches as cb
import schur_ref as sr
import test_gpu_stage_ref as stage
from test_gpu_stage_ref import _case

pytestmark = pytest.mark.gpu


def _scene(name):
    from bundleadjustmentmatlab_amd.scene import make_config
    s = cb.CR32 if name == "cr32" else cb.SCENES[name]
    sc = make_config("cfg2", **cb.scene_kw(s))
    return (sc,) + stage._obs(sc)


def _without_camera(name, j):
    sc, pt, cam, ox = _scene(name)
    keep = cam != j
    return sc, pt[keep], cam[keep], ox[keep]


def _is(n):
    return lambda got: got == n


def _route64(s):
    """The 64-row route's plan facts and launch counts."""
    lv = cb.levels(s["tiles"])

    def plan(p):
        return (p["cr_levels"] == len(lv) and p["cr_rows"] == cb.TILE and p["tiles"] == s["tiles"]
                and p["cr_elim"] == s["tiles"] and p["cr_keep"] == sum(nk for _, nk in lv)
                and p["nd_arcs"] == 0)
    launches = dict(k_cr_factor=_is(len(lv)), k_cr_update=_is(cb.update_launches(lv)),
                    k_cr_back=_is(len(lv)), k_factor_step=_is(0))
    return dict(plan=plan, launches=launches)


# the projective scene's lambda: the smallest of 1e-3 / 1e-2 / 1e-1 at which
# LAPACK's Cholesky of the same S succeeds
LAM = {"na12-t5-m700": 1e-3}
CASES = {}
for _name, _s in cb.SCENES.items():
    _kw = dict(model="projective") if _s["na"] == 12 else {}
    CASES["cr64/" + _name] = _case((lambda nm: lambda: _scene(nm))(_name), na=_s["na"],
                                   lam=LAM.get(_name, 1e-3), **_route64(_s), **_kw)
MASKS = {
    "cr64/pivot-na6-t9-m43": _case(lambda: _scene("na6-t9-m43"), fixed=(0, 1), pivot="first2",
                                   **_route64(cb.SCENES["na6-t9-m43"])),
    "cr64/unseen31-na10-t6-m64": _case(lambda: _without_camera("na10-t6-m64", 31), na=10,
                                       fixed=(31,), **_route64(cb.SCENES["na10-t6-m64"])),
}
CASES.update(MASKS)
SCENE_OF = {"cr64/" + k: k for k in cb.SCENES}
SCENE_OF.update({"cr64/pivot-na6-t9-m43": "na6-t9-m43", "cr64/unseen31-na10-t6-m64": "na10-t6-m64"})


def _cr32_plan(p):
    return (p["cr_levels"] == cb.CR32["levels"] and p["cr_rows"] == 30
            and p["cr_elim"] == cb.CR32["tiles"])


CR32 = {
    "cr32/one-launch": _case(lambda: _scene("cr32"), plan=_cr32_plan,
                             launches=dict(k_cr_factor=_is(1), k_cr_back=_is(0),
                                           k_factor_step=_is(0))),
    "cr32/levels": _case(lambda: _scene("cr32"), plan=_cr32_plan, env={"VLGBA_CR_FUSED": "0"},
                         launches=dict(k_cr_factor=_is(cb.CR32["levels"]),
                                       k_cr_back=_is(cb.CR32["levels"]), k_factor_step=_is(0))),
}
CASES.update(CR32)


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _banded_lapack(m, na, jk, blocks, e_, band):
    """LAPACK's banded Cholesky solve (dpbsv) of the symmetrised S in fp64;
    None when S is not positive definite."""
    import scipy.linalg as sl
    ab = np.zeros((band + 1, na * m))
    r, c = np.meshgrid(np.arange(na), np.arange(na), indexing="ij")
    i = (na * jk[:, 0])[:, None, None] + r[None]
    j = (na * jk[:, 1])[:, None, None] + c[None]
    low = i >= j
    assert (i - j)[low].max() <= band
    ab[(i - j)[low], j[low]] = np.asarray(blocks)[low]
    try:
        return sl.solveh_banded(ab, np.asarray(e_, dtype=np.float64), lower=True)
    except np.linalg.LinAlgError:
        return None


def _checks(r, key):
    """test_solve_stage's assertions but the residual: (fixed cameras, rows)."""
    na, m = r["na"], r["m"]
    assert r["info"].chol_failed == 0 and r["info"].pinv == 0, key
    fixed = np.zeros(m, dtype=bool)
    fixed[list(r["fixed"])] = True
    assert np.all(r["da"][:, fixed] == 0.0), key
    assert np.all(np.isfinite(r["da"])), key
    return fixed, np.repeat(~fixed, na)


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("cr64/")])
def test_solve_stage_64_rows(gpu, oracle, key):
    r = stage._run(gpu, key, CASES)
    name = SCENE_OF[key]
    s = cb.SCENES[name]
    na, m, ld = r["na"], r["m"], r["na"] * r["m"]
    ncu, lv = _ncu(), cb.levels(s["tiles"])
    kinds = cb.kinds64(lv, ncu)
    print(f"CR-BRANCH route {key}: ld {ld} tiles {r['plan']['tiles']} cr_rows "
          f"{r['plan']['cr_rows']} levels {r['plan']['cr_levels']} on {ncu} compute units: "
          f"{' '.join(kinds)} (factor, update; s split, u unsplit); launches {r['counts']}")
    stage._facts(r, key, CASES)
    large = name in cb.LARGE
    if large:
        assert kinds == s["kinds"], (
            f"{key}: a device of {ncu} compute units does not take level 0 through the unsplit "
            f"bodies this case is here for (wanted {s['kinds']}, got {kinds})")
    fixed, rows = _checks(r, key)
    bar = ld * sr.U53
    eta = sr.residual_blocks(m, na, r["jk"], r["blocks"], r["e"], r["da"], rows)
    band = na * s["track"] - 1
    if large:
        x = _banded_lapack(m, na, r["jk"], r["blocks"], r["e"], band)
        ref = "not positive definite" if x is None else \
            f"{sr.residual_blocks(m, na, r['jk'], r['blocks'], r['e'], x, rows) / bar:.3g}"
        print(f"CR-BRANCH solve {key}: lambda {r['lam']:g} ld {ld} eta / (ld u) GPU "
              f"{eta / bar:.3g} LAPACK banded (dpbsv) {ref}; blockwise residual, the dense "
              f"figure is left out")
    else:
        S = np.zeros((ld, ld))
        for (j, k), B in zip(r["jk"], r["blocks"]):
            S[na * j:na * j + na, na * k:na * k + na] = np.tril(B) if j == k else B
        dense = sr.residual(S, r["e"], r["da"], rows)
        lapack = sr.residual(S, r["e"], oracle.chol_solve_fixed(S, r["e"]), rows)
        print(f"CR-BRANCH solve {key}: ld {ld} eta / (ld u) GPU {eta / bar:.3g} (dense "
              f"{dense / bar:.3g}) LAPACK {lapack / bar:.3g}")
        assert abs(eta - dense) <= sr.residual_slack(2 * band + 1, dense), (key, eta, dense)
        assert dense <= bar, (key, dense / bar)
    assert eta <= bar, (key, eta / bar)


@pytest.mark.parametrize("key", list(CR32))
def test_solve_stage_32_rows_past_the_compute_units(gpu, key):
    r = stage._run(gpu, key, CASES)
    na, m, ld = r["na"], r["m"], r["na"] * r["m"]
    ncu, lv = _ncu(), cb.levels(cb.CR32["tiles"])
    ne0, nrec = lv[0][0], cb.CR32["tiles"]
    took = dict(l0two=cb.cr32_l0two(ne0, ncu), factor_split=cb.cr32_factor_split(ne0, ncu),
                back_one_launch=cb.cr32_back_one_launch(nrec, ncu))
    print(f"CR-BRANCH route {key}: ld {ld} tiles {nrec} cr_rows {r['plan']['cr_rows']} levels "
          f"{r['plan']['cr_levels']} on {ncu} compute units: {took}; launches {r['counts']}")
    stage._facts(r, key, CASES)
    assert took == dict(l0two=True, factor_split=False, back_one_launch=False), (
        f"{key}: a device of {ncu} compute units does not take the large-count branches this "
        f"case is here for: {took}")
    _, rows = _checks(r, key)
    bar = ld * sr.U53
    eta = sr.residual_blocks(m, na, r["jk"], r["blocks"], r["e"], r["da"], rows)
    x = _banded_lapack(m, na, r["jk"], r["blocks"], r["e"], na * cb.CR32["track"] - 1)
    ref = sr.residual_blocks(m, na, r["jk"], r["blocks"], r["e"], x, rows)
    print(f"CR-BRANCH solve {key}: ld {ld} eta / (ld u) GPU {eta / bar:.3g} LAPACK banded (dpbsv) "
          f"{ref / bar:.3g}; blockwise residual, the dense figure is left out")
    assert eta <= bar, (key, eta / bar)


def test_32_row_routes_agree_bit_for_bit(gpu):
    """(tests/test_gpu_parity.py::test_cr_one_launch_bit_identical's claim on
    the runs above: it costs nothing here.)"""
    a, b = (stage._run(gpu, k, CASES) for k in CR32)
    assert np.array_equal(a["da"], b["da"]) and np.array_equal(a["db"], b["db"])


@pytest.mark.parametrize("name", ["na7-t8-m75", "na6-t9-m1400"])
def test_no_state_between_solves(gpu, name):
    s = cb.SCENES[name]
    na = s["na"]
    sc, pt, cam, ox = _scene(name)
    m, ld = sc.m, na * sc.m
    a, b = stage._params(sc, na)
    bar = ld * sr.U53
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, na, lambda0=1e-3) as ba:
        ba.set_params(a, b)
        jk, blocks, e_ = (x.copy() for x in ba.reduced_system(dense=False))
        plan = ba.plan_info()
        assert plan["cr_levels"] == len(s["kinds"]) and plan["cr_rows"] == cb.TILE, plan
        steps, infos = [], []
        for _ in range(2):
            infos.append(ba.step(relinearize=False, update_lm=False))
            steps.append([x.copy() for x in ba.last_step()])
        eta = [sr.residual_blocks(m, na, jk, blocks, e_, st[0]) for st in steps]
        # an applied LM step, then the solve of the new linearisation
        applied = ba.step(relinearize=True, update_lm=True)
        jk3, blocks3, e3 = (x.copy() for x in ba.reduced_system(dense=False))
        third = ba.step(relinearize=False, update_lm=False)
        da3 = ba.last_step()[0].copy()
    eta3 = sr.residual_blocks(m, na, jk3, blocks3, e3, da3)
    print(f"CR-BRANCH repeat {name}: ld {ld} eta / (ld u) first {eta[0] / bar:.3g} second "
          f"{eta[1] / bar:.3g}; applied step accepted {applied.accepted} lambda "
          f"{infos[0].lambda_:g} -> {third.lambda_:g}; third solve {eta3 / bar:.3g}")
    assert all(i.chol_failed == 0 and i.pinv == 0 for i in infos + [applied, third])
    assert np.array_equal(steps[0][0], steps[1][0]), "da of the second solve"
    assert np.array_equal(steps[0][1], steps[1][1]), "db of the second solve"
    assert max(eta) <= bar
    assert applied.accepted == 1 and np.array_equal(jk3, jk) and not np.array_equal(blocks3, blocks)
    assert np.all(np.isfinite(da3)) and eta3 <= bar, eta3 / bar
