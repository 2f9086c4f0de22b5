"""The fast path's track-length thresholds and long-track machinery against the
references of tests/test_gpu_stage_ref.py (whose harness, cases table shape,
checks and bars are taken over unchanged), on the planted scenes of
tests/track_scenes.py (proven on the CPU by tests/test_track_scenes.py; the
references' bounds at these track lengths by tests/test_schur_ref.py).

Ladders (m = 280, two tracks of every length on a threshold: BA_MF_CMAX(na) | +1,
8 | 9, 32 | 33, 90 | 91, 128 | 129, 256 | 257, and the longest): three full
segments per track, the second trip of k_long_db's loop, k_long_y / k_long_db /
k_schur_long_acc / k_schur_reduce's pair loop / the segment chunks of the
linearisation for num_a 6, 7, 9, 10 and 12, ndb = num_a (nomex; the radial
camera always).
    ladder-6 (top 257), ladder-7 (257), ladder-10 (273), ladder-10-over (274),
    ladder-10-nomex (273), ladder-12 (projective, 280), ladder-9 (radial, 304
    cameras, top 303), ladder-9-over (radial, 304 cameras, top 304)
Shared (m = 100, C tracks of 91..100 views through cameras 0..89): per-camera
long lists and per-block pair counts of C = 48 | 49 (BA_LMATCH_BATCH), 64 | 65
(k_long_pairs' second round), 256 | 257 (BA_LCAM_LDS: the sequential merge),
num_a 6; C = 257 also at num_a 9, 10 and 12.
Every case runs with VLGBA_LONG_ACC=1 and =0; the two routes' reduced system
and step are bit-identical.  Plan facts of every case: ordered == 0,
reordered == 1, 0 < mfma_groups < groups, long_points == the planted tracks of
at least 91 views.

A. Schur / solve / update: the three checks of test_gpu_stage_ref.py.
B. linearisation of the ladders: W bit-identical to the oracle's, V / eB and
   U / eA at test_long_tracks_fast_path's 1e-13 bars.  The oracle has no
   radial camera: the num_a = 9 ladders' residuals and U, eA, V, eB, W are held
   to the propagated bounds of tests/radial_ref.py instead (|diff| / bound <= 1,
   as tests/test_gpu_radial.py does on its scenes).
C. k_point_cov on the ladders (first two cameras pivot) as
   test_gpu_covariance.py::test_point_stage: all three bins; the workgroup
   launch stages its W rows in LDS up to 273 views at num_a 10 (65520 B) and
   reads global memory at 274 (65760 B > BA_COV_LDS); at num_a 9 the edge is
   303 | 304 views (65448 B | 65664 B).

A long double reference is computed once per scene and shared by the two
routes after their inputs were compared bit for bit (they are the same
linearisation); where they differ it is computed again.  The slowest case is
shared-257's Schur reference (1.1 M terms): 1.7 / 4.6 / 6.6 s at num_a 6 / 10 /
12 beside the MI355X, every other case under 2 s -- the planted counts are
what the case is for, so they stay.

Every test prints its figures before it asserts (lines starting TRACK-REF,
pytest -s).  Measured on an MI355X; no bar was widened.  The two
VLGBA_LONG_ACC routes gave the same figures in every case (they are
bit-identical), so each is listed once.

Largest |diff| / bound per stage:
    case               S        e_       db (planted tracks alone)
    ladder-6           0.29     0.070    0.040 (0.012)
    ladder-7           0.36     0.036    0.046 (0.012)
    ladder-10          0.28     0.046    0.056 (0.035)
    ladder-10-over     0.28     0.044    0.047 (0.028)
    ladder-10-nomex    0.28     0.046    0.040 (0.014)
    ladder-12          0.23     0.059    0.056 (0.036)
    ladder-9           0.24     0.018    0.028 (0.014)
    ladder-9-over      0.27     0.023    0.040 (0.016)
    shared-48          0.076    0.0028   0.067 (0.0016)
    shared-49          0.056    0.011    0.051 (0.0021)
    shared-64          0.051    0.0033   0.038 (0.0018)
    shared-65          0.060    0.016    0.044 (0.0018)
    shared-256         0.028    0.0037   0.045 (0.0024)
    shared-257         0.027    0.0026   0.046 (0.0029)
    shared-257-na10    0.027    0.0033   0.044 (0.0015)
    shared-257-na12    0.030    0.0029   0.044 (0.0023)
    shared-257-na9     0.029    0.0030   0.033 (0.00092)
eta / (ld u) of the solve, GPU | LAPACK Cholesky on the same S:
    ladder-6 (ld 1680) 0.0019 | 0.0020, ladder-7 (1960) 0.0017 | 0.0021,
    ladder-10 and -nomex (2800) 0.0013 | 0.0013, ladder-10-over 0.0013 | 0.0013,
    ladder-12 (3360) 0.0010 | 0.0011, shared-49 (600) 0.0046 | 0.0074,
    shared-257 0.0047 | 0.0058, ladder-9 (2736) 0.0015 | 0.0018, ladder-9-over
    0.0014 | 0.0016, shared-257-na9 (900) 0.0038 | 0.0037.
Linearisation: W bit-identical in all five ladders; max |diff| / max |ref| of
    V 4.5e-16 .. 9.5e-16, eB 2.4e-16 .. 1.3e-15, U 2.6e-16 .. 4.3e-16,
    eA 1.6e-16 .. 5.1e-16 (the bars are 1e-13).  The radial ladders, largest
    |diff| / bound: ladder-9 U 0.098 eA 0.083 V 0.051 eB 0.046 W 0.15, residuals
    0.17; ladder-9-over U 0.097 eA 0.085 V 0.051 eB 0.046 W 0.15, residuals 0.19.
Point covariances, largest |diff| / bound: ladder-6 0.057, ladder-7 0.051,
    ladder-10 0.0041 (65520 B of W rows, in LDS), ladder-10-over 0.0032
    (65760 B, from global memory), ladder-9 0.033 (65448 B, in LDS),
    ladder-9-over 0.033 (65664 B, from global memory); planted lengths up to 8 took the 8-lane
    launch, 9 .. 32 one wave, 33 and more one workgroup.
"""
import numpy as np
import pytest

import cov_ref as cr
import schur_ref as sr
import test_gpu_stage_ref as stage
import track_scenes as ts
from test_gpu_stage_ref import _case, _environ, _params

pytestmark = pytest.mark.gpu

ROUTES = ("1", "0")                    # VLGBA_LONG_ACC
# name: (num_a, longest track, constructor keywords)
LADDER = {
    "ladder-6": (6, 257, {}),
    "ladder-7": (7, 257, {}),
    "ladder-10": (10, 273, {}),
    "ladder-10-over": (10, 274, {}),
    "ladder-10-nomex": (10, 273, dict(semantics="nomex")),
    "ladder-12": (12, 280, dict(model="projective")),
    # the radial camera on 304 cameras: k_point_cov's LDS edge at num_a = 9 is 303 | 304 views
    "ladder-9": (9, 303, {}),
    "ladder-9-over": (9, 304, {}),
}
LADDER_M = {"ladder-9": 304, "ladder-9-over": 304}      # cameras, where not ladder()'s 280
# name: (num_a, C, constructor keywords)
SHARED = {f"shared-{C}": (6, C, {}) for C in (48, 49, 64, 65, 256, 257)}
SHARED["shared-257-na10"] = (10, 257, {})
SHARED["shared-257-na12"] = (12, 257, dict(model="projective"))
SHARED["shared-257-na9"] = (9, 257, {})
SHARED_SOLVE = ["shared-49", "shared-257", "shared-257-na9"]   # the solve does not depend on C
# restated from ba_internal.h
COV_T8, COV_T64, COV_LDS = 8, 32, 65536


def _scene(name):
    if name in LADDER:
        return ts.ladder(LADDER[name][0], LADDER[name][1], m=LADDER_M.get(name, 280))
    return ts.shared(SHARED[name][1])


def _long_points(name):
    sc, pt, _, _ = _scene(name)
    return int(ts.is_long(np.bincount(pt, minlength=sc.n)).sum())


def _plan(name):
    def ok(p):
        return (p["ordered"] == 0 and p["reordered"] == 1
                and 0 < p["mfma_groups"] < p["groups"]
                and p["long_points"] == _long_points(name))
    return ok


# lambda: the ladders run at 0.1 and not at the harness's 1e-3, where the step
# of the num_a 7 and 10 ladders is REJECTED -- by the CPU oracle's pass too
# (cost 2319 -> 2729 and 2613 -> 3574: the MEX back substitution leaves out the
# calibration terms of db); at 0.1 the oracle accepts every ladder's step, and
# an accepted step is what the update check's a + da, b + db needs.
LAM = {"ladder": 0.1, "shared": 1e-3}
CASES = {}
for _name, (_na, _, _kw) in dict(LADDER, **SHARED).items():
    for _v in ROUTES:
        CASES[f"{_name}/acc{_v}"] = _case((lambda nm: lambda: _scene(nm))(_name), na=_na,
                                          lam=LAM[_name.split("-")[0]],
                                          env={"VLGBA_LONG_ACC": _v}, plan=_plan(_name), **_kw)


def _keys(names):
    return [f"{nm}/acc{v}" for nm in names for v in ROUTES]


def _run(gpu, key):
    r = stage._run(gpu, key, CASES)
    stage._facts(r, key, CASES)
    name = key.split("/")[0]
    if name in SHARED:
        assert r["plan"]["long_points"] == SHARED[name][1], (key, r["plan"])
    else:      # every planted track of at least 91 views, two of each length
        want = 2 * sum(k >= 91 for k in ts.ladder_lengths(*LADDER[name][:2]))
        assert r["plan"]["long_points"] == want, (key, r["plan"])
    return r


_MEMO = {}


def _memo(tag, inputs, fn):
    """fn() once per tag while the inputs stay the same bit for bit (the two
    routes of a case share one linearisation: one reference)."""
    inputs = [np.asarray(x) for x in inputs]
    if tag in _MEMO:
        old, val = _MEMO[tag]
        if len(old) == len(inputs) and all(np.array_equal(x, y) for x, y in zip(old, inputs)):
            return val
    val = fn()
    _MEMO[tag] = ([x.copy() for x in inputs], val)
    return val


# ---------------------------------------------------------------------------
# A. the three stages
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_schur_stage(gpu, key):
    r = _run(gpu, key)
    L, lam = r["lin"], r["lam"]
    ref = _memo(("schur", key.split("/")[0]), [L[k] for k in ("W", "V", "eB", "U", "eA")],
                lambda: sr.schur(r["m"], r["n"], r["na"], r["pt"], r["cam"], L["W"], L["V"],
                                 L["eB"], L["U"], L["eA"], lam))
    got = set(map(tuple, r["jk"].tolist()))
    nz = np.flatnonzero(np.any(ref["S"] != 0, axis=(1, 2)))
    missing = [tuple(ref["jk"][q]) for q in nz if tuple(ref["jk"][q]) not in got]
    rs, re = sr.schur_ratio(ref, r["jk"], r["blocks"], r["e"])
    print(f"TRACK-REF schur {key}: S {rs:.3g} e_ {re:.3g} of the bound "
          f"({len(r['jk'])} blocks, most points {ref['npts'].max()}, long_points "
          f"{r['plan']['long_points']})")
    assert not missing, (key, missing[:5])
    assert rs <= 1.0 and re <= 1.0, (key, rs, re)


@pytest.mark.parametrize("key", _keys(list(LADDER) + SHARED_SOLVE))
def test_solve_stage(gpu, oracle, key):
    r = _run(gpu, key)
    na, m = r["na"], r["m"]
    assert r["info"].chol_failed == 0 and r["info"].pinv == 0, key
    ld = na * m
    S = np.zeros((ld, ld))
    for (j, k), B in zip(r["jk"], r["blocks"]):
        S[na * j:na * j + na, na * k:na * k + na] = np.tril(B) if j == k else B
    da = r["da"]
    assert np.all(np.isfinite(da))
    bar = ld * sr.U53
    eta = sr.residual(S, r["e"], da)
    eta_lapack = _memo(("lapack", key.split("/")[0]), [r["jk"], r["blocks"], r["e"]],
                       lambda: sr.residual(S, r["e"], oracle.chol_solve_fixed(S, r["e"])))
    print(f"TRACK-REF solve {key}: ld {ld} eta / (ld u) GPU {eta / bar:.3g} "
          f"LAPACK {eta_lapack / bar:.3g}")
    assert eta <= bar, (key, eta / bar, eta_lapack / bar)


@pytest.mark.parametrize("key", list(CASES))
def test_update_stage(gpu, key):
    r = _run(gpu, key)
    na, L = r["na"], r["lin"]
    ndb = na if r["kw"].get("semantics") == "nomex" or na == 9 else 6   # radial: all nine rows
    Vinv = _memo(("vinv", key.split("/")[0]), [L["V"]], lambda: sr.vinv_of(L["V"], r["lam"]))
    ref, bound = sr.back_subst(na, ndb, r["pt"], r["cam"], L["W"], Vinv, L["eB"], r["da"])
    ratio = sr.db_ratio(r["db"], ref, bound)
    # the planted tracks alone (k_long_db for the long ones)
    first = _scene(key.split("/")[0])[0].base_n
    lratio = sr.db_ratio(r["db"][:, first:], ref[:, first:], bound[:, first:])
    print(f"TRACK-REF update {key}: db {ratio:.3g} of the bound (planted tracks {lratio:.3g})")
    assert ratio <= 1.0, (key, ratio)
    assert np.all(np.bincount(r["pt"], minlength=r["n"]) > 0)
    if ndb > 6:      # the terms past the sixth are not nothing in this case
        assert np.abs(r["da"].reshape(na, -1, order="F")[6:]).max() > 0
    assert r["info2"].accepted == 1, key
    assert np.array_equal(r["a2"], r["a"] + r["da2"]), key
    assert np.array_equal(r["b2"], r["b"] + r["db2"]), key


@pytest.mark.parametrize("name", list(LADDER) + list(SHARED))
def test_long_acc_routes_bit_identical(gpu, name):
    """k_schur_long_acc against k_schur_reduce's own pair loop: the reduced
    system and both steps of one case, bit for bit (tests/test_gpu_long_acc.py
    claims it for num_a 6 and 7 on tracks of up to 220 views)."""
    r1, r0 = (_run(gpu, f"{name}/acc{v}") for v in ROUTES)
    for k in ("jk", "blocks", "e", "da", "db", "da2", "db2", "a2", "b2"):
        assert np.array_equal(r1[k], r0[k]), (name, k)
    for k in ("W", "V", "eB", "U", "eA"):
        assert np.array_equal(r1["lin"][k], r0["lin"][k]), (name, k)
    for k in ("groups", "mfma_groups", "long_points", "cr_levels", "nd_arcs"):
        assert r1["plan"][k] == r0["plan"][k], (name, k)


# ---------------------------------------------------------------------------
# B. the linearisation of the ladders
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder-6", "ladder-7", "ladder-10", "ladder-10-over",
                                  "ladder-12"])
def test_linearisation(gpu, oracle, poracle, name):
    r = _run(gpu, f"{name}/acc1")
    sc, pt, cam, ox = _scene(name)
    na, lin = r["na"], r["lin"]
    if na == 12:
        X = np.zeros((2, sc.n, sc.m), order="F")
        X[0, pt, cam], X[1, pt, cam] = ox[:, 0], ox[:, 1]
        vis = np.zeros((sc.n, sc.m), order="F")
        vis[pt, cam] = 1.0
        out = poracle.mex1(r["a"], r["b"], X, vis)
        ref = dict(U=out[4], V=out[5], W=out[6][:, :, pt, cam], eA=out[7], eB=out[8])
    else:
        pb = oracle.SparseProblem(sc.m, sc.n, pt, cam, ox, sc.K)
        ref = oracle.sp_linearize(pb, r["a"], r["b"], na)
        ref["W"] = np.asfortranarray(ref["W"].T).reshape(na, 3, -1, order="F")
    fig = {nm: float(np.max(np.abs(lin[nm] - ref[nm])) / np.max(np.abs(ref[nm])))
           for nm in ("V", "eB", "U", "eA")}
    print(f"TRACK-REF linearise {name}: W equal {np.array_equal(lin['W'], ref['W'])}; "
          "max |diff| / max |ref| " + " ".join(f"{k} {v:.2g}" for k, v in fig.items()))
    assert np.array_equal(lin["W"], ref["W"]), name
    for nm in ("V", "eB"):
        assert np.allclose(lin[nm], ref[nm], rtol=1e-13, atol=1e-13 * np.abs(ref[nm]).max()), nm
    for nm in ("U", "eA"):
        assert np.max(np.abs(lin[nm] - ref[nm])) <= 1e-13 * np.max(np.abs(ref[nm])), nm


@pytest.mark.parametrize("name", ["ladder-9", "ladder-9-over"])
def test_linearisation_radial(gpu, name):
    """The oracle has no radial camera: the ladder's residuals and its
    linearisation (the segment chunks of the 129-, 257-, 303- and 304-view
    tracks at num_a = 9) within the propagated bounds of tests/radial_ref.py, as
    tests/test_gpu_radial.py::test_linearisation_within_the_reference_bounds."""
    import radial_ref as ra
    import robust_ref as rr
    r = _run(gpu, f"{name}/acc1")
    sc, pt, cam, _ = _scene(name)
    a, b, ox = stage._radial(sc, pt, cam)
    assert np.array_equal(a, r["a"]) and np.array_equal(b, r["b"])
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 9, lambda0=r["lam"]) as ba:
        ba.set_params(a, b)
        lin = ba.linearization()
        e = ba.residuals()[0]
    for k in ("U", "eA", "V", "eB", "W"):      # the case's own linearisation is this one
        assert np.array_equal(lin[k], r["lin"][k]), (name, k)
    eref, eb = ra.residuals(sc.K, a, b, pt, cam, ox)
    R = ra.linearization(sc.K, a, b, pt, cam, e, sc.m, sc.n)
    fig = {k: rr.ratio(lin[k], R[k], R[k + "_b"]) for k in ("U", "eA", "V", "eB", "W")}
    fig["e"] = rr.ratio(e, eref, eb)
    first = int(np.searchsorted(pt, sc.base_n))
    planted = rr.ratio(lin["W"][:, :, first:], R["W"][:, :, first:], R["W_b"][:, :, first:])
    print(f"TRACK-REF linearise {name}: largest |diff| / bound "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items())
          + f" (W of the planted tracks {planted:.3g}; longest track {np.bincount(pt).max()})")
    assert np.all(np.abs(lin["W"][6:9]).max(axis=(1, 2)) > 0)       # f, k1, k2 rows alive
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


# ---------------------------------------------------------------------------
# C. the covariance's point stage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder-6", "ladder-7", "ladder-10", "ladder-10-over",
                                  "ladder-9", "ladder-9-over"])
def test_point_cov(gpu, name):
    na = LADDER[name][0]
    sc, pt, cam, ox = _scene(name)
    if na == 9:
        a, b, ox = stage._radial(sc, pt, cam)
    else:
        a, b = _params(sc, na)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, na, pivot=np.arange(sc.m) < 2) as ba:
        ba.set_params(a, b)
        L = ba.linearization()
        cov = ba.covariance(scale=False, full=True)
        plan = ba.plan_info()
    assert plan["ordered"] == 0 and plan["long_points"] == _long_points(name), plan
    track = np.bincount(pt, minlength=sc.n)
    lad = track[sc.base_n:]
    bins = {"8 lanes": sorted(set(lad[lad <= COV_T8].tolist())),
            "one wave": sorted(set(lad[(lad > COV_T8) & (lad <= COV_T64)].tolist())),
            "one workgroup": sorted(set(lad[lad > COV_T64].tolist()))}
    need = 8 * int(track.max()) * 3 * na
    staged = need <= COV_LDS
    Vi = sr.vinv_of(L["V"], 0.0)
    ref, bound = cr.point_cov(na, pt, cam, L["W"], Vi, cov["full"])
    ratio = cr.point_ratio(cov["pts"], ref, bound)
    lratio = cr.point_ratio(cov["pts"][:, :, sc.base_n:], ref[:, :, sc.base_n:],
                            bound[:, :, sc.base_n:])
    print(f"TRACK-REF point cov {name}: {ratio:.3g} of the bound (planted tracks {lratio:.3g}); "
          f"bins {bins}; the workgroup launch's W rows: {need} B, "
          f"{'staged in LDS' if staged else 'read from global memory'}")
    assert all(bins.values()) and 8 in bins["8 lanes"] and 9 in bins["one wave"]
    assert 32 in bins["one wave"] and 33 in bins["one workgroup"]
    assert staged == (not name.endswith("-over"))
    if na == 10:
        assert need == (65520 if staged else 65760)
    if na == 9:
        assert need == (65448 if staged else 65664)
    pts = cov["pts"]
    assert np.array_equal(pts, pts.transpose(1, 0, 2)), name
    assert np.all(track > 0) and np.all(np.isfinite(pts))
    assert ratio <= 1.0, (name, ratio)
