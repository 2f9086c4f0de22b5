"""The selected covariance method (VLGBA_COV_SELECTED: a selected inverse on
the camera-aligned cyclic reduction's factors, k_cr32_selinv) on the GPU, held
to the references of tests/test_gpu_covariance.py: every stage is fed the
GPU's own upstream outputs and prints its figures before it asserts (lines
starting COVSEL, pytest -s).

Scenes: banded cfg2 scenes with n = 40 m points and tracks of G + 1 cameras (G =
32 // num_a cameras per reduction tile), the first two cameras as pivot, sized
for the reduction's tile-count edges -- 2 tiles, 3 with a one-camera last tile,
4, 5 and 9 tiles (4 levels) -- at num_a 6, 7, 10 and 12 (projective,
fix_structure, no pivot), one deeper case (num_a 6, 81 cameras: 17 tiles, 5
levels, ld 486: past LD_MAX, so its reference follows test_gpu_covariance's
rule for that), fix_motion, fix_structure, and the scene with unseen and
single-view points.

1. camera stage   cam and every co-visible block against the reference inverse
                  of the long double S0 formed from the GPU's linearisation;
                  bar 8 x the same figure of numpy.linalg.inv on the fp64-formed
                  S0 (the reference route's own floor); exact symmetry, exact
                  zeros on fixed rows; fixed_rows, sse, dof, sigma2 bit for bit
                  the dense method's on a twin context.
2. point stage    pts within cov_ref.point_cov's per-entry bound, the reference
                  fed the returned blocks scattered into a symmetric matrix.
3. dense getter   the dense method's blocks are the same entries of its full.
4. state          two calls bit-identical; step, selected covariance, step,
                  step == step, step, step on a twin; last_step unchanged;
                  scale multiplies by sigma2.
5. memory         scratch_bytes <= 3 * 32 * 32 * 8 * ceil(ld / cr_rows) (the
                  library exposes no allocator accounting: the figure the call
                  reports is what is checked).
6. rejections     contexts without the camera-aligned reduction, ordered,
                  parity, sharded; full=True; a gauge-free scene.
7. drivers        bundle_euclid_obs(covariance_method="selected").

Measured on an MI355X; no bar was widened.

1. co-visible blocks (diagonal blocks), GPU | numpy.linalg.inv on the
   fp64-formed S0; tiles / levels, cond(S0):
    sel6-10     9.3e-12 | 1.4e-11  (4.5e-12 | 7.2e-12)   2 / 2   3.9e7
    sel6-11     1.1e-11 | 1.1e-11  (1.0e-11 | 7.9e-12)   3 / 2   5.9e7
    sel6-20     2.4e-10 | 2.7e-10  (1.9e-10 | 2.0e-10)   4 / 3   2.8e8
    sel6-21     1.8e-10 | 3.9e-10  (1.8e-10 | 3.2e-10)   5 / 3   2.7e8
    sel6-41     1.8e-10 | 1.1e-09  (1.7e-10 | 8.8e-10)   9 / 4   6.5e8
    sel6-81     9.6e-10 | 1.4e-09  (8.6e-10 | 1.1e-09)   17 / 5  5.8e9
    sel7-8      2.8e-11 | 3.8e-11  (1.8e-11 | 2.9e-11)   2 / 2   3.3e9
    sel7-9      7.1e-11 | 5.6e-11  (5.4e-11 | 4.3e-11)   3 / 2   4.8e9
    sel7-33     1.4e-10 | 1.1e-10  (1.4e-10 | 1.1e-10)   9 / 4   8.1e10
    sel10-6     4.1e-11 | 1.6e-10  (3.8e-11 | 1.4e-10)   2 / 2   1.7e10
    sel10-7     1.8e-10 | 2.9e-10  (1.7e-10 | 2.9e-10)   3 / 2   3.6e10
    sel10-25    3.4e-08 | 3.1e-08  (3.0e-08 | 3.0e-08)   9 / 4   9.8e11
    sel12-4     8.3e-05 | 1.1e-03                        2 / 2   1.2e18
    sel12-5     8.9e-05 | 7.9e-04                        3 / 2   1.4e18
    sel12-17    9.1e-05 | 1.7e-04                        9 / 4   2.8e18
    sel-fix-motion 0 | 0;  sel-fix-structure 1.6e-14 | 8.9e-15
    sel-unseen-single  2.7e-10 | 9.1e-10  (2.7e-10 | 7.9e-10)
   The largest GPU / numpy ratio is 1.75 (sel-fix-structure); the bar is 8.
2. largest |diff| / bound: 0.0013 (sel10-25) .. 0.036 (sel-unseen-single);
   sel6-81 0.028; the projective, fix-motion and fix-structure cases exact.
3. selected against dense, diagonal blocks: 8.8e-14 (sel6-10) .. 1.6e-10
   (sel10-25); projective 1.0e-4 .. 2.4e-4 (cond 1e18).
6. the gauge-free scene returned 0 with largest |Sigma_a| 8.1e3.
"""
import numpy as np
import pytest

import cov_ref as cr
import schur_ref as sr
import test_gpu_covariance as tc
from test_gpu_stage_ref import ROWS, TRACK, _banded, _ladybug, _params, _unseen_single

pytestmark = pytest.mark.gpu


def _scene(na, m, n=None):
    def make():
        from bundleadjustmentmatlab_amd.scene import make_config
        sc = make_config("cfg2", m=m, n=n or 40 * m, track=TRACK[na], seed=41)
        return sc, sc.obs_pt, sc.obs_cam, sc.obs_x
    return make


CASES = {}
for _na, _ms in ((6, (10, 11, 20, 21, 41)), (7, (8, 9, 33)), (10, (6, 7, 25))):
    for _m in _ms:
        CASES[f"sel{_na}-{_m}"] = tc._case(_scene(_na, _m), na=_na)
for _m in (4, 5, 17):
    CASES[f"sel12-{_m}"] = tc._case(_scene(12, _m), na=12, pivot=False, fix_structure=True,
                                    model="projective")
CASES["sel6-81"] = tc._case(_scene(6, 81, 2000))
CASES["sel-fix-motion"] = tc._case(_scene(6, 11), fix_motion=True)
CASES["sel-fix-structure"] = tc._case(_scene(6, 11), pivot=False, fix_structure=True)
CASES["sel-unseen-single"] = tc._case(_unseen_single)
STATE_KEYS = ["sel6-21", "sel6-41", "sel10-7"]


def _make(gpu, key):
    """test_gpu_covariance._make on this file's cases."""
    tc.CASES[key] = CASES[key]
    try:
        return tc._make(gpu, key)
    finally:
        del tc.CASES[key]


def _is_cr32(ba, na):
    p = ba.plan_info()
    return p["cr_levels"] > 0 and p["cr_rows"] == ROWS[na]


_RUNS = {}


def _run(gpu, key):
    """One selected and one dense (twin) context per case, shared by the tests."""
    if key in _RUNS:
        if isinstance(_RUNS[key], BaseException):    # never run a failed case again
            pytest.fail(f"{key}: the case's run failed in an earlier test: {_RUNS[key]!r}")
        return _RUNS[key]
    try:
        ba, r = _make(gpu, key)
        with ba:
            ba.set_params(r["a"], r["b"])
            r["plan"] = ba.plan_info()
            assert _is_cr32(ba, r["na"]), (key, r["plan"])
            r["lin"] = ba.linearization()
            ba.set_covariance_method("selected")
            assert ba.get_covariance_method() == "selected"
            r["cov"] = ba.covariance(scale=False, blocks=True)
            r["cov2"] = ba.covariance(scale=False, blocks=True)
            r["covs"] = ba.covariance(scale=True, blocks=True)
        twin, _ = _make(gpu, key)
        with twin:
            twin.set_params(r["a"], r["b"])
            assert twin.get_covariance_method() == "dense"
            r["dense"] = twin.covariance(scale=False, full=True, blocks=True)
            r["denses"] = twin.covariance(scale=True, full=True, blocks=True)
        _RUNS[key] = r
    except BaseException as exc:
        _RUNS[key] = exc
        raise
    return r


def _block_stack(full, jk, na):
    """(na, na, nb) blocks (j, k) of a dense matrix."""
    return np.stack([full[na * j:na * j + na, na * k:na * k + na] for j, k in jk], axis=2)


def _scatter(jk, blocks, na, m):
    """The co-visible blocks [b, r, c] as a symmetric (na m, na m) matrix."""
    S = np.zeros((na * m, na * m))
    for (j, k), B in zip(jk, blocks):
        S[na * j:na * j + na, na * k:na * k + na] = B
        S[na * k:na * k + na, na * j:na * j + na] = B.T
    return S


@pytest.mark.parametrize("key", list(CASES))
def test_camera_stage(gpu, key):
    r = _run(gpu, key)
    ref, cov, na, m = tc._camera_ref(r, "selected:" + key), r["cov"], r["na"], r["m"]
    jk, fixed = cov["blk_jk"], ref["fixed"]
    got = cov["blocks"].transpose(1, 2, 0)
    want_b, inv64_b = _block_stack(ref["want"], jk, na), _block_stack(ref["inv64"], jk, na)
    fig_blk = cr.block_figure(got, want_b, na)
    floor_blk = cr.block_figure(inv64_b, want_b, na)
    fig_diag = cr.block_figure(cov["cam"], cr.diag_blocks(ref["want"], na), na)
    ntile = -(-na * m // ROWS[na])
    print(f"COVSEL camera {key}: ld {na * m} tiles {ntile} levels {r['plan']['cr_levels']} "
          f"fixed rows {int(fixed.sum())} cond(S0) {ref['cond']:.2g}: diagonal blocks GPU "
          f"{fig_diag:.3g} numpy {ref['floor_diag']:.3g}; co-visible blocks GPU {fig_blk:.3g} "
          f"numpy {floor_blk:.3g}; ms camera {cov['ms'][0]:.3f} points {cov['ms'][1]:.3f} "
          f"(dense {r['dense']['ms'][0]:.3f})")
    cam = cov["cam"]
    assert np.array_equal(cam, cam.transpose(1, 0, 2)), key
    fx = fixed.reshape(m, na)
    for j in range(m):
        assert np.all(cam[fx[j], :, j] == 0.0) and np.all(cam[:, fx[j], j] == 0.0), (key, j)
    for (j, k), B in zip(jk, cov["blocks"]):
        assert np.all(B[fx[j], :] == 0.0) and np.all(B[:, fx[k]] == 0.0), (key, j, k)
        if j == k:
            assert np.array_equal(B, cam[:, :, j]), (key, j)
    assert np.all(np.isfinite(cam)) and np.all(np.isfinite(cov["blocks"]))
    dense = r["dense"]
    assert cov["fixed_rows"] == int(fixed.sum()) == dense["fixed_rows"], key
    for k in ("sse", "dof", "sigma2"):
        assert cov[k] == dense[k], (key, k)
    assert fig_diag <= 8 * ref["floor_diag"] and fig_blk <= 8 * floor_blk, key


@pytest.mark.parametrize("key", list(CASES))
def test_point_stage(gpu, key):
    r = _run(gpu, key)
    na, L, cov = r["na"], r["lin"], r["cov"]
    Vi = sr.vinv_of(L["V"], 0.0)
    full = _scatter(cov["blk_jk"], cov["blocks"], na, r["m"])
    ref, bound = cr.point_cov(na, r["pt"], r["cam"], L["W"], Vi, full)
    ratio = cr.point_ratio(cov["pts"], ref, bound)
    track = np.bincount(r["pt"], minlength=r["n"])
    print(f"COVSEL points {key}: {ratio:.3g} of the bound (longest track {track.max()}, "
          f"{int((track == 0).sum())} unseen)")
    pts = cov["pts"]
    assert np.array_equal(pts, pts.transpose(1, 0, 2)), key
    assert np.all(pts[:, :, track == 0] == 0.0), key
    if r["kw"].get("fix_structure"):
        assert np.all(pts == 0.0), key
    if r["kw"].get("fix_motion"):
        low = np.tril(np.ones((3, 3), dtype=bool))[:, :, None]
        assert np.array_equal(pts, np.where(low, Vi, Vi.transpose(1, 0, 2))), key
        assert np.all(cov["blocks"] == 0.0)
    assert np.all(np.isfinite(pts))
    assert ratio <= 1.0, (key, ratio)


@pytest.mark.parametrize("key", list(CASES))
def test_dense_blocks_are_entries_of_full(gpu, key):
    """vlgba_get_covariance_blocks on the dense method: the same entries as its
    full matrix, bit for bit, scaled or not, in the reduced system's order."""
    r = _run(gpu, key)
    na = r["na"]
    for d in (r["dense"], r["denses"]):
        assert np.array_equal(d["blk_jk"], r["cov"]["blk_jk"]), key
        assert np.array_equal(d["blocks"].transpose(1, 2, 0),
                              _block_stack(d["full"], d["blk_jk"], na)), key
    # ... and the selected method's differ from them by rounding only
    fig = cr.block_figure(r["cov"]["cam"], r["dense"]["cam"], na)
    print(f"COVSEL dense-vs-selected {key}: diagonal blocks {fig:.3g}")


@pytest.mark.parametrize("key", list(CASES))
def test_calls_repeat_and_scale(gpu, key):
    r = _run(gpu, key)
    cov, cov2, covs = r["cov"], r["cov2"], r["covs"]
    for k in ("cam", "pts", "blocks"):
        assert np.array_equal(cov[k], cov2[k]), (key, k)
        assert np.array_equal(covs[k], cov[k] * cov["sigma2"]), (key, k)
    for k in ("sse", "dof", "sigma2", "fixed_rows", "scratch_bytes"):
        assert cov[k] == cov2[k] == covs[k], (key, k)
    assert cov["dof"] > 0 and cov["sigma2"] == cov["sse"] / cov["dof"], key
    # memory: three 32 x 32 fp64 tiles per reduction tile, no dense ld^2 scratch
    na, m = r["na"], r["m"]
    ntile = -(-na * m // ROWS[na])
    assert 0 < cov["scratch_bytes"] <= 3 * 32 * 32 * 8 * ntile, key
    assert r["dense"]["scratch_bytes"] == 8 * (na * m) ** 2, key


@pytest.mark.parametrize("key", STATE_KEYS)
def test_step_after_call_is_bit_identical(gpu, key):
    """step, selected covariance, step, step against step, step, step on a twin
    context (the one-launch reduction with its default folds); the last step
    read back after the call is the one before it."""
    out = []
    for with_cov in (True, False):
        ba, r = _make(gpu, key)
        with ba:
            ba.set_params(r["a"], r["b"])
            p = ba.plan_info()
            assert _is_cr32(ba, r["na"]) and p["camupd_fold"] == 1 and p["vinv_fold"] == 1, p
            i1 = ba.step(relinearize=True, update_lm=True)
            s1 = [x.copy() for x in ba.last_step()]
            if with_cov:
                ba.covariance(method="selected")
                assert ba.get_covariance_method() == "dense"
                for x, y in zip(s1, ba.last_step()):
                    assert np.array_equal(x, y), key
            i2 = ba.step(relinearize=True, update_lm=True)
            s2 = [x.copy() for x in ba.last_step()]
            i3 = ba.step(relinearize=False, update_lm=True)
            s3 = [x.copy() for x in ba.last_step()]
            prm = ba.get_params()
        out.append(([i1, i2, i3], s1 + s2 + s3 + list(prm)))
    (ia, xa), (ib, xb) = out
    for a, b in zip(ia, ib):
        for f, _ in a._fields_:
            assert getattr(a, f) == getattr(b, f), (key, f)
    assert ia[0].accepted == 1
    for a, b in zip(xa, xb):
        assert np.array_equal(a, b), key


def _rejects(gpu, ba):
    with pytest.raises(gpu._lib.VlgbaError, match=r"\(-1001\)"):
        ba.set_covariance_method("selected")
    assert ba.get_covariance_method() == "dense"


def test_rejections(gpu):
    na = 6
    # no camera-aligned reduction: the mixed ladybug scene
    sc, pt, cam, ox = _ladybug(m=40, n=1500, max_track=30, radius=150.0, seed=23)
    a, b = _params(sc, na)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, na, pivot=np.arange(sc.m) < 2) as ba:
        ba.set_params(a, b)
        assert not _is_cr32(ba, na)
        _rejects(gpu, ba)
        with pytest.raises(gpu._lib.VlgbaError, match=r"\(-1001\)"):
            ba.covariance(method="selected")
        assert np.all(np.isfinite(ba.covariance(method="dense")["cam"]))
    sc, pt, cam, ox = _banded(na, 33)
    a, b = _params(sc, na)
    piv = np.arange(sc.m) < 2
    for kw in (dict(ordered=1), dict(parity=True),
               dict(rank=0, world_size=2, allreduce=lambda arr: None)):
        with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, na, pivot=piv, **kw) as ba:
            _rejects(gpu, ba)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, na, pivot=piv) as ba:
        ba.set_params(a, b)
        assert _is_cr32(ba, na)
        assert ba._L.vlgba_get_covariance_blocks(ba._h, None, None) == -1001   # before a call
        with pytest.raises(gpu._lib.VlgbaError, match=r"\(-1001\)"):
            ba.covariance(full=True, method="selected")
        assert ba.get_covariance_method() == "dense"
        with pytest.raises(ValueError):
            ba.covariance(method="sparse")
        sel = ba.covariance(method="selected", blocks=True)
        dense = ba.covariance(full=True, method="dense", blocks=True)
        assert np.array_equal(sel["blk_jk"], dense["blk_jk"])
        fig = cr.block_figure(sel["cam"], dense["cam"], na)
        print(f"COVSEL banded6-33 dense-vs-selected: diagonal blocks {fig:.3g}")
        assert np.all(np.isfinite(dense["full"]))


def test_gauge_free_scene(gpu):
    """Nothing fixed: S0 is singular up to the Jacobians' noise, so the call
    returns finite output or VLGBA_E_SINGULAR and nothing else, and the context
    steps afterwards."""
    sc, pt, cam, ox = _scene(6, 10)()
    a, b = _params(sc, 6)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 6) as ba:
        ba.set_params(a, b)
        assert _is_cr32(ba, 6)
        ba.set_covariance_method("selected")
        try:
            cov = ba.covariance(scale=False, blocks=True)
        except gpu._lib.VlgbaError as exc:
            print(f"COVSEL gauge-free: {exc}")
            assert "(-1007)" in str(exc)
        else:
            print(f"COVSEL gauge-free: 0, largest |Sigma_a| {np.abs(cov['blocks']).max():.3g}")
            assert all(np.all(np.isfinite(cov[k])) for k in ("cam", "pts", "blocks"))
        info = ba.step()
        assert np.isfinite(info.new_sse)


def test_driver_covariance_method(gpu):
    """bundle_euclid_obs(return_covariance=True, covariance_method="selected")
    appends the dict of a BundleAdjuster set to the returned parameters."""
    sc, pt, cam, ox = _banded(6, 33)
    opts = ("fix_calibration", "fix_pivot", [1, 2])
    out = gpu.bundle_euclid_obs(sc.K, sc.T0, sc.w0, sc.X0, pt, cam, ox, *opts,
                                return_covariance=True, covariance_method="selected")
    K_, Te_, w_, Xe_, err, cov = out
    plain = gpu.bundle_euclid_obs(sc.K, sc.T0, sc.w0, sc.X0, pt, cam, ox, *opts)
    assert all(np.array_equal(x, y) for x, y in zip(plain, out[:5]))
    a = np.asfortranarray(np.vstack([w_, Te_]))
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 6, pivot=np.arange(sc.m) < 2) as ba:
        ba.set_params(a, np.asfortranarray(Xe_[:3]))
        ba.set_covariance_method("selected")
        want = ba.covariance()
    for k in ("cam", "pts"):
        assert np.array_equal(cov[k], want[k]), k
    for k in ("sse", "dof", "sigma2", "fixed_rows", "scratch_bytes"):
        assert cov[k] == want[k], k
    assert cov["scratch_bytes"] == 3 * 32 * 32 * 8 * -(-6 * sc.m // 30)
    assert np.all(cov["cam"][:, :, :2] == 0.0) and np.all(np.diagonal(cov["cam"][:, :, 2:]) > 0)
