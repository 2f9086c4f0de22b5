"""The default fast path, stage by stage and entry by entry, against the
extended-precision reference of tests/schur_ref.py (proven on the CPU by
tests/test_schur_ref.py).  Every stage is fed the GPU's OWN upstream outputs,
so a stage is judged alone:

A. Schur   k_schur_mfma / k_schur_group -> k_schur_reduce (-> k_schur_long_acc):
           every block of vlgba_get_reduced_system and e_ within the per-entry
           rounding bound of the long double S / e_ formed from the getter's
           U, V, W, eA, eB; every non-zero block of the reference returned.
B. solve   one-launch / per-level cyclic reduction, envelope, nested
           dissection, dense tiles, sequential: componentwise backward error
           eta of da in the GPU's own S da = e_ at most ld * u (Cholesky's
           backward-error scale with constant 1; ld = num_a * m).  The solvers
           read the ASSEMBLED tiles (k_assemble_tiles, or k_schur_reduce's
           direct writes), the getter the block sums: a small eta proves the
           assembly too.  Fixed cameras have da == 0 exactly.
C. update  k_update_linearize's db within the bound of the long double back
           substitution with the GPU's da; an accepted step's parameters are
           a + da, b + db bit for bit.

Shapes: n = 1327 (prime: partial MFMA K-blocks and a partial last chunk);
m = 33 / 33 / 34 / 33 cameras for num_a = 6 / 7 / 10 / 12 (camera-aligned CR
tiles of 5 / 4 / 3 / 2 cameras: the last tile is partial), and m = 32 for 6.
The radial camera (num_a = 9: parameters and observations through the lens as
tests/test_gpu_radial.py, all nine rows of da in the back substitution) has
27-row CR tiles of three cameras: m = 34 / 33 / 35 leave one / three / two
cameras in the last tile.

The solve stage runs all five solvers on every banded shape (auto in the
stage cases; per-level CR, envelope, dense, sequential beside them), nd and
envelope on a 120-camera loop-closure scene.  The routes are pinned by plan
facts and by the launch counts of one timed pass (k_assemble; k_cr_factor).

Every test prints its figures before it asserts (lines starting STAGE-REF,
pytest -s).  Measured on an MI355X; no bar was widened.

Largest |diff| / bound per stage:
    S     banded 0.0008 .. 0.0012 (MFMA and terms, num_a 6 / 7 / 9 / 10 / 12;
          num_a 9: 0.0011 .. 0.0012, e_ 0.0004 .. 0.0008, db 0.019 .. 0.020);
          lambda 10: 0.014; mixed plan 0.18; tracks of 10: 0.0008;
          long tracks 0.30 (k_schur_long_acc and k_schur_reduce's pairs:
          the same), one point in 140 cameras 0.091; two cameras, one
          point 0.031; pivot 0.0007; fix_motion / fix_structure exact
    e_    0.0002 .. 0.0014; lambda 10: 0.0089; two cameras, one point 0.030
    db    0.017 .. 0.078 (largest: single-view points; lambda 10: 0.074);
          unseen points and fix_structure exactly 0

eta / (ld u) of the solve, GPU | LAPACK Cholesky on the same S:
    shape (ld)             CR one launch   CR per level    envelope        dense           sequential
    num_a  6, m 33 (198)   0.019 | 0.0096  0.019 | 0.0096  0.052 | 0.0096  0.052 | 0.0096  0.016 | 0.0096
    num_a  6, m 32 (192)   0.026 | 0.0090  0.026 | 0.0090  0.042 | 0.0090  0.042 | 0.0090  0.020 | 0.0090
    num_a  7, m 33 (231)   0.015 | 0.0071  0.015 | 0.0071  0.023 | 0.0071  0.023 | 0.0071  0.014 | 0.0071
    num_a  9, m 34 (306)   0.0065 | 0.0047 0.0065 | 0.0047 0.0083 | 0.0047 0.0083 | 0.0047 0.011 | 0.0047
    num_a 10, m 34 (340)   0.0091 | 0.0050 0.0091 | 0.0050 0.013 | 0.0050  0.013 | 0.0050  0.011 | 0.0050
    num_a 12, m 33 (396)   0.0082 | 0.0038 0.0082 | 0.0038 0.012 | 0.0038  0.012 | 0.0038  0.0055 | 0.0038
    ladybug, m 120 (720)   nd 0.0080 | 0.0047              0.0088 | 0.0047
    the same, num_a 9 (1080) nd 0.0080 | 0.0036            0.0082 | 0.0036
    num_a 9, one-launch CR: m 33 (297) 0.011 | 0.0063, m 35 (315) 0.0078 | 0.0054,
    terms 0.0095 | 0.0055, pivot 0.015 | 0.0078
    other auto cases: lambda 10 0.020 | 0.015, terms 0.015 | 0.014, mixed
    0.012 | 0.0094, tracks of 10 0.030 | 0.010, long tracks 0.0036 | 0.0035,
    140-camera point 0.012 | 0.0038, unseen camera 0.030 | 0.033, single-view
    points 0.037 | 0.025, two cameras 0.068 | 0.094, pivot 0.012 | 0.011,
    fix_structure 0.0094 | 0.013; the worst GPU solve is 0.068 of the bar.
"""
import contextlib
import os

import numpy as np
import pytest

import schur_ref as sr

pytestmark = pytest.mark.gpu

TRACK = {6: 6, 7: 5, 9: 4, 10: 4, 12: 3}   # G + 1 cameras: S tridiagonal in G-camera tiles
ROWS = {na: na * (32 // na) for na in TRACK}   # the whole cameras that fit a 32-row CR tile


def _params(sc, na):
    a = np.zeros((na, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if na == 7:
        a[6] = sc.K[0]
    elif na == 10:
        a[6:10] = sc.K
    return a, np.asfortranarray(sc.X0[:3])


def _radial(sc, pt, cam):
    """The radial camera (num_a = 9) on a scene, as tests/test_gpu_radial.py::_rscene:
    (a (9, m), b, observations): the scene's perturbed poses and points with
    coefficients 10 % / 20 % off the truth, and the true scene's observations
    through the lens (k1 = -0.15, k2 = 0.03) plus 0.5 px noise."""
    import radial_ref as ra
    kt = np.tile(np.array(ra.K_TRUE)[:, None], (1, sc.m))
    ox = ra.observe(sc.K, ra.pack(sc.K, sc.w, sc.T, kt), sc.X, pt, cam, 0.5, 77)
    a = ra.pack(sc.K, sc.w0, sc.T0, kt * np.array([[0.9], [1.2]]))
    return a, np.asfortranarray(sc.X0[:3]), ox


def _obs(sc):
    return sc.obs_pt, sc.obs_cam, sc.obs_x


def _banded(na, m):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=m, n=1327, track=TRACK[na], seed=41)
    return (sc,) + _obs(sc)


def _ladybug(**kw):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("ladybug", **kw)
    return (sc,) + _obs(sc)


def _cfg3_t10():
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg3", m=40, n=2000, seed=6, track=10)
    return (sc,) + _obs(sc)


def _long_edge():
    """tests/test_gpu_edge.py::test_track_longer_than_chunk_cap's scene: point 0
    seen by all 140 cameras."""
    from bundleadjustmentmatlab_amd.scene import make_config, project
    sc = make_config("cfg2", m=140, n=2000, seed=5)
    allc = np.arange(sc.m)
    extra, z = project(sc.K, sc.w, sc.T, sc.X, allc, np.zeros(sc.m, dtype=int))
    assert np.all(z > 0)
    keep = sc.obs_pt != 0
    pt = np.r_[np.zeros(sc.m, int), sc.obs_pt[keep]].astype(np.int32)
    cam = np.r_[allc, sc.obs_cam[keep]].astype(np.int32)
    ox = np.r_[np.asarray(extra).reshape(sc.m, 2), sc.obs_x[keep]]
    order = np.lexsort((cam, pt))
    return sc, pt[order], cam[order], ox[order]


def _no_camera5():
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=12, n=400, seed=3)
    keep = sc.obs_cam != 5
    return sc, sc.obs_pt[keep], sc.obs_cam[keep], sc.obs_x[keep]


def _unseen_single():
    """Points 0..9 unseen, points 10..59 seen by one camera."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=10, n=300, seed=4)
    first = np.r_[True, sc.obs_pt[1:] != sc.obs_pt[:-1]]
    keep = ~(sc.obs_pt < 10) & ~((sc.obs_pt >= 10) & (sc.obs_pt < 60) & ~first)
    return sc, sc.obs_pt[keep], sc.obs_cam[keep], sc.obs_x[keep]


def _two_one():
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=2, n=1, seed=7)
    return (sc,) + _obs(sc)


LONG = dict(m=160, n=1200, max_track=30, radius=150.0, seed=29, long_frac=0.01,
            long_len=(130, 150))


def _case(scene, na=6, lam=1e-3, env=None, plan=None, fixed=(), launches=None, **kw):
    """launches: {timer name: predicate on its launch count in one timed pass}."""
    return dict(scene=scene, na=na, lam=lam, env=env or {}, plan=plan or (lambda p: True),
                fixed=fixed, launches=launches or {}, kw=kw)


# launch counts of one pass that tell the routes apart: the direct assembly
# launches no k_assemble; the one-launch CR is one k_cr_factor, the per-level
# CR one per level.  (k_schur_long_acc has no timer of its own -- it runs
# inside k_schur_reduce's -- so VLGBA_LONG_ACC's two routes are told apart
# only by the variable itself, spelt as ba_solver.cpp's setup_long_pairs reads it.)
_ONE = lambda n: n == 1          # noqa: E731
_NONE = lambda n: n == 0         # noqa: E731
_MANY = lambda n: n > 1          # noqa: E731
FUSED = {"k_cr_factor": _ONE}
LEVELS = {"k_cr_factor": _MANY}


def _cr(na):
    return lambda p: p["cr_levels"] > 0 and p["cr_rows"] == ROWS[na]


def _mfma_cr(na):
    return lambda p: p["mfma"] == 1 and _cr(na)(p)


def _terms_cr(na):
    return lambda p: p["mfma"] == 0 and p["mfma_groups"] == 0 and _cr(na)(p)


# the cases of all three stages
STAGE = {
    "banded6-m33": _case(lambda: _banded(6, 33), plan=_mfma_cr(6),
                         launches=dict(FUSED, k_assemble=_NONE)),
    "banded6-m33-lam10": _case(lambda: _banded(6, 33), lam=10.0, plan=_mfma_cr(6)),
    "banded6-m32": _case(lambda: _banded(6, 32), plan=_mfma_cr(6),
                         launches=dict(FUSED, k_assemble=_NONE)),
    "banded6-m33-terms": _case(lambda: _banded(6, 33), plan=_terms_cr(6), schur_kernel="terms"),
    "banded6-m33-assemble": _case(lambda: _banded(6, 33), plan=_mfma_cr(6),
                                  launches=dict(FUSED, k_assemble=_ONE),
                                  env={"VLGBA_ASM_DIRECT": "0"}),
    "banded7-m33": _case(lambda: _banded(7, 33), na=7, plan=_mfma_cr(7), launches=FUSED),
    "banded7-m33-terms": _case(lambda: _banded(7, 33), na=7, plan=_terms_cr(7),
                               schur_kernel="terms"),
    "banded10-m34": _case(lambda: _banded(10, 34), na=10, plan=_mfma_cr(10), launches=FUSED),
    "banded10-m34-terms": _case(lambda: _banded(10, 34), na=10, plan=_terms_cr(10),
                                schur_kernel="terms"),
    "projective12-m33": _case(lambda: _banded(12, 33), na=12, plan=_mfma_cr(12),
                              launches=FUSED, model="projective"),
    "mixed": _case(lambda: _ladybug(m=40, n=1500, max_track=30, radius=150.0, seed=23),
                   plan=lambda p: 0 < p["mfma_groups"] < p["groups"]),
    "tracks10": _case(_cfg3_t10, plan=lambda p: p["mfma"] == 0 and p["ordered"] == 0),
    "long-acc": _case(lambda: _ladybug(**LONG), env={"VLGBA_LONG_ACC": "1"},
                      plan=lambda p: p["long_points"] > 0 and p["ordered"] == 0),
    "long-reduce": _case(lambda: _ladybug(**LONG), env={"VLGBA_LONG_ACC": "0"},
                         plan=lambda p: p["long_points"] > 0 and p["ordered"] == 0),
    "long-140": _case(_long_edge, plan=lambda p: p["long_points"] == 1 and p["ordered"] == 0),
    "camera-unseen": _case(_no_camera5, fixed=(5,)),
    "points-unseen-single": _case(_unseen_single),
    "two-cameras-one-point": _case(_two_one),
    "pivot": _case(lambda: _banded(6, 33), plan=_mfma_cr(6), fixed=(0, 1), pivot="first2"),
    "fix-motion": _case(lambda: _banded(6, 33), fixed="all", fix_motion=True),
    "fix-structure": _case(lambda: _banded(6, 33), fix_structure=True),
    "nomex10": _case(lambda: _banded(10, 34), na=10, plan=_mfma_cr(10), semantics="nomex"),
    # the radial camera: 27-row CR tiles of three cameras; the last tile holds
    # one camera (m = 34), three (m = 33), two (m = 35)
    "radial9-m34": _case(lambda: _banded(9, 34), na=9, plan=_mfma_cr(9), launches=FUSED),
    "radial9-m34-terms": _case(lambda: _banded(9, 34), na=9, plan=_terms_cr(9),
                               schur_kernel="terms"),
    "radial9-m33": _case(lambda: _banded(9, 33), na=9, plan=_mfma_cr(9), launches=FUSED),
    "radial9-m35": _case(lambda: _banded(9, 35), na=9, plan=_mfma_cr(9), launches=FUSED),
    "radial9-pivot": _case(lambda: _banded(9, 34), na=9, plan=_mfma_cr(9), fixed=(0, 1),
                           pivot="first2"),
}
# the solve stage alone: the other four solvers on every banded shape, and
# the nested-dissection order (tests/test_gpu_nd.py's scene)
_NOCR = lambda p: p["cr_levels"] == 0 and p["nd_arcs"] == 0    # noqa: E731
SOLVE = {}
for _name, _na, _m in (("banded6-m33", 6, 33), ("banded6-m32", 6, 32), ("banded7-m33", 7, 33),
                       ("banded10-m34", 10, 34), ("projective12-m33", 12, 33),
                       ("radial9-m34", 9, 34)):
    _kw = dict(model="projective") if _na == 12 else {}
    _sc = (lambda na, m: lambda: _banded(na, m))(_na, _m)
    SOLVE[_name + "-levels"] = _case(_sc, na=_na, plan=_cr(_na), launches=LEVELS,
                                     env={"VLGBA_CR_FUSED": "0"}, **_kw)
    for _solver in ("envelope", "dense", "sequential"):
        SOLVE[f"{_name}-{_solver}"] = _case(_sc, na=_na, plan=_NOCR, solver=_solver,
                                            launches={"k_cr_factor": _NONE}, **_kw)
SOLVE["ladybug120-nd"] = _case(lambda: _ladybug(m=120, n=12000, seed=3), solver="nd",
                               plan=lambda p: p["nd_arcs"] >= 2 and p["cr_levels"] == 0)
SOLVE["ladybug120-envelope"] = _case(lambda: _ladybug(m=120, n=12000, seed=3), plan=_NOCR,
                                     solver="envelope")
SOLVE["ladybug120-nd-na9"] = _case(lambda: _ladybug(m=120, n=12000, seed=3), na=9, solver="nd",
                                   plan=lambda p: p["nd_arcs"] >= 2 and p["cr_levels"] == 0)
SOLVE["ladybug120-envelope-na9"] = _case(lambda: _ladybug(m=120, n=12000, seed=3), na=9,
                                         plan=_NOCR, solver="envelope")
CASES = dict(STAGE, **SOLVE)
# the update stage's list: banded 6 / 10, mixed, long tracks, nomex, unseen
# points and fix_structure (db == 0 exactly), the masks
UPDATE = ["banded6-m33", "banded6-m33-lam10", "banded10-m34", "mixed", "long-acc", "long-140",
          "nomex10", "points-unseen-single", "fix-structure", "pivot", "tracks10",
          "radial9-m34", "radial9-pivot"]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def _run(gpu, key, cases=None):
    """One context per case, shared by the stages' tests (nothing here is
    modified afterwards): the linearisation, the reduced system, the step at
    the same linearisation, then an LM-applied step and its parameters.
    cases: another module's case table (keys of its own), default CASES."""
    if key in _RUNS:
        if isinstance(_RUNS[key], BaseException):    # never run a failed case again
            pytest.fail(f"{key}: the case's run failed in an earlier test: {_RUNS[key]!r}")
        return _RUNS[key]
    try:
        _RUNS[key] = _run_case(gpu, key, cases)
    except BaseException as exc:
        _RUNS[key] = exc
        raise
    return _RUNS[key]


def _run_case(gpu, key, cases=None):
    c = (cases or CASES)[key]
    sc, pt, cam, ox = c["scene"]()
    na, kw = c["na"], dict(c["kw"])
    m, n = sc.m, sc.n
    if kw.get("model") == "projective":
        from bundleadjustmentmatlab_amd.scene import projective_from
        Pp, Xp = projective_from(sc)
        a, b = np.asfortranarray(Pp.reshape(12, m, order="F")), np.asfortranarray(Xp[0:3])
        K, kw["m"] = None, m
    elif na == 9:
        (a, b, ox), K = _radial(sc, pt, cam), sc.K
    else:
        (a, b), K = _params(sc, na), sc.K
    if isinstance(kw.get("pivot"), str):
        kw["pivot"] = np.arange(m) < 2
    with _environ(c["env"]):
        ba = gpu.BundleAdjuster(K, pt, cam, ox, n, na, lambda0=c["lam"], **kw)
    with ba:
        ba.set_params(a, b)
        lin = ba.linearization()
        jk, blocks, e_ = ba.reduced_system(dense=False)
        info = ba.step(relinearize=False, update_lm=False)
        da, db = ba.last_step()
        plan = ba.plan_info()
        info2 = ba.step(relinearize=False, update_lm=True)
        da2, db2 = ba.last_step()
        a2, b2 = ba.get_params()
        launches = {}
        if c["launches"]:
            ba.set_timing(True)
            ba.kernel_ms(reset=True)
            ba.step(relinearize=True, update_lm=False)
            km = ba.kernel_ms(reset=True)
            launches = {k: km.get(k, (0.0, 0))[1] for k in c["launches"]}
    r = dict(c, m=m, n=n, pt=pt, cam=cam, a=a, b=b, lin=lin, jk=jk.copy(), blocks=blocks.copy(),
             e=e_.copy(), info=info, da=da.copy(), db=db.copy(), plan=plan, info2=info2,
             da2=da2.copy(), db2=db2.copy(), a2=a2.copy(), b2=b2.copy(), counts=launches)
    return r


def _facts(r, key, cases=None):
    """The plan facts that prove the intended kernels ran."""
    c = (cases or CASES)[key]
    assert c["plan"](r["plan"]), (key, r["plan"])
    for k, ok in c["launches"].items():
        assert ok(r["counts"][k]), (key, k, r["counts"])
    assert r["info"].lambda_ == c["lam"]


@pytest.mark.parametrize("key", list(STAGE))
def test_schur_stage(gpu, key):
    r = _run(gpu, key)
    _facts(r, key)
    L = r["lin"]
    ref = sr.schur(r["m"], r["n"], r["na"], r["pt"], r["cam"], L["W"], L["V"], L["eB"], L["U"],
                   L["eA"], r["lam"])
    # every non-zero block of the reference is among the returned ones
    got = set(map(tuple, r["jk"].tolist()))
    nz = np.flatnonzero(np.any(ref["S"] != 0, axis=(1, 2)))
    missing = [tuple(ref["jk"][q]) for q in nz if tuple(ref["jk"][q]) not in got]
    assert not missing, (key, missing[:5])
    rs, re = sr.schur_ratio(ref, r["jk"], r["blocks"], r["e"])
    print(f"STAGE-REF schur {key}: S {rs:.3g} e_ {re:.3g} of the bound "
          f"({len(r['jk'])} blocks, most points {ref['npts'].max()})")
    assert rs <= 1.0 and re <= 1.0, (key, rs, re)


@pytest.mark.parametrize("key", list(CASES))
def test_solve_stage(gpu, oracle, key):
    r = _run(gpu, key)
    _facts(r, key)
    na, m = r["na"], r["m"]
    assert r["info"].chol_failed == 0 and r["info"].pinv == 0, key
    ld = na * m
    S = np.zeros((ld, ld))
    for (j, k), B in zip(r["jk"], r["blocks"]):
        S[na * j:na * j + na, na * k:na * k + na] = np.tril(B) if j == k else B
    fixed = np.zeros(m, dtype=bool)
    fixed[list(range(m)) if r["fixed"] == "all" else list(r["fixed"])] = True
    da = r["da"]
    assert np.all(da[:, fixed] == 0.0), key
    assert np.all(np.isfinite(da))
    rows = np.repeat(~fixed, na)
    bar = ld * sr.U53
    eta = sr.residual(S, r["e"], da, rows)
    eta_lapack = sr.residual(S, r["e"], oracle.chol_solve_fixed(S, r["e"]), rows)
    print(f"STAGE-REF solve {key}: ld {ld} eta / (ld u) GPU {eta / bar:.3g} "
          f"LAPACK {eta_lapack / bar:.3g}")
    assert eta <= bar, (key, eta / bar, eta_lapack / bar)


@pytest.mark.parametrize("key", UPDATE)
def test_update_stage(gpu, key):
    r = _run(gpu, key)
    _facts(r, key)
    na, L = r["na"], r["lin"]
    # (the radial camera's back substitution takes all nine rows of da under
    # either semantics: ba_solver.cpp's ctx_options, ndb of the radial model)
    ndb = na if r["kw"].get("semantics") == "nomex" or na == 9 else 6
    Vinv = sr.vinv_of(L["V"], r["lam"])
    ref, bound = sr.back_subst(na, ndb, r["pt"], r["cam"], L["W"], Vinv, L["eB"], r["da"])
    ratio = sr.db_ratio(r["db"], ref, bound)
    print(f"STAGE-REF update {key}: db {ratio:.3g} of the bound")
    assert ratio <= 1.0, (key, ratio)
    seen = np.bincount(r["pt"], minlength=r["n"]) > 0
    assert np.all(r["db"][:, ~seen] == 0.0)
    if r["kw"].get("fix_structure"):
        assert np.all(r["db"] == 0.0)
    # the LM-applied step from the same linearisation: accepted, and the new
    # parameters are the fp64 sums a + da, b + db (mex_bundle_3_db_new.c:
    # 133-145) bit for bit; pivot cameras do not move
    assert r["info2"].accepted == 1, key
    assert np.array_equal(r["a2"], r["a"] + r["da2"]), key
    assert np.array_equal(r["b2"], r["b"] + r["db2"]), key
    for j in ([] if r["fixed"] == "all" else r["fixed"]):
        assert np.array_equal(r["a2"][:, j], r["a"][:, j]), key
