"""vlgba_covariance on the GPU, stage by stage, against tests/cov_ref.py (proven
on the CPU by tests/test_cov_ref.py).  As in test_gpu_stage_ref.py every stage
is fed the GPU's OWN upstream outputs and prints its figures before it asserts
(lines starting COV, pytest -s).

A. camera stage   Sigma_a = S0^-1 (dense assembly, unit-diagonal rule, rocSOLVER
                  dpotrf + dpotri, k_cov_finish) against inverse_ld of the long
                  double S0 that schur_ref.schur(lam = 0) forms from the
                  getter's linearisation.  Figure: the largest per-block
                  max|diff| / max|reference block| over the diagonal blocks
                  and over all blocks.  Bar: 8 x the same figure of
                  numpy.linalg.inv on the fp64 S0 -- an S0 FORMED in fp64 from
                  the same linearisation (cov_ref.schur_fp64), as the GPU's is:
                  it carries the Schur complement's own fp64 rounding, which
                  cond(S0) amplifies like the inversion's (the long double S0
                  rounded to fp64 does not, and would hold the GPU to an
                  accuracy no fp64 Schur complement has).  long-140 (ld 840) is
                  past what inverse_ld does in a few seconds: its reference is
                  numpy.linalg.inv of the long double S0 rounded to fp64.
B. point stage    k_point_cov against cov_ref.point_cov fed the GPU's returned
                  cov_a_full, the getter's W and schur_ref.vinv_of(V, 0): every
                  entry within its rounding bound (ratio <= 1), exact symmetry,
                  exact zeros for unseen points and under fix_structure,
                  Sigma_b = V+ exactly under fix_motion (the correction's bound
                  is zero there).
C. end to end     banded6 and banded10 against numpy.linalg.inv of the full
                  normal matrix built from the GPU's linearisation; bar 8 x the
                  two-route fp64 floor of the references alone (the full
                  inverse against the fp64 Schur route), as test_cov_ref.py.
D. state          step, covariance, step == step, step on a twin context bit
                  for bit (default, ordered and parity mode); the reduced
                  system and the last step are unchanged by a call; two calls
                  are bit-identical; scale multiplies by sigma2 = SSE / dof;
                  the drivers' return_covariance.

Measured on an MI355X; no bar was widened.

A. all blocks (diagonal blocks), GPU | numpy.linalg.inv on the fp64-formed S0:
    banded6     1.1e-09 | 7.9e-10  (5.5e-10 | 3.6e-10)   cond(S0) 5.2e8
    banded7     1.6e-10 | 5.6e-10  (1.5e-10 | 2.4e-10)   8.4e10
    banded10    3.5e-08 | 5.3e-08  (2.2e-08 | 2.5e-08)   2.1e12
    mixed       1.4e-12 | 7.5e-12  (9.1e-13 | 2.8e-12)   6.9e7
    long-140    3.0e-09 | 5.5e-09  (1.6e-09 | 2.7e-09)   1.2e10
    points-unseen-single  2.7e-10 | 9.1e-10  (2.7e-10 | 7.9e-10)
    fix-motion  0 | 0;  fix-structure 1.5e-14 | 1.2e-14
    projective12-fix-structure  2.0e-04 | 2.5e-04   cond(S0) 3e18
    banded6 ordered / parity    8.0e-10 | 8.6e-10  (3.8e-10 | 3.7e-10)
B. largest |diff| / bound: banded6 0.018, banded7 0.0072, banded10 0.0014,
   mixed 0.062, long-140 0.017, points-unseen-single 0.029, ordered / parity
   0.016; fix-motion, fix-structure and projective12-fix-structure exact.
   (k_point_cov adds each term with one fma; with separate products and sums
   the same cases gave 0.016, 0.0073, 0.0023, 0.11, 0.018, 0.032, 0.013.)
C. GPU | floor: banded6 cameras 2.4e-09 | 4.9e-10, points 9.2e-10 | 1.2e-09;
   banded10 cameras 2.8e-08 | 6.4e-08, points 1.2e-08 | 3.3e-07.
D. two-cameras-one-point returned VLGBA_E_SINGULAR.
"""
import numpy as np
import pytest

import cov_ref as cr
import schur_ref as sr
from test_gpu_stage_ref import (_banded, _ladybug, _long_edge, _params, _two_one,
                                _unseen_single)

pytestmark = pytest.mark.gpu


def _case(scene, na=6, pivot=True, **kw):
    return dict(scene=scene, na=na, pivot=pivot, kw=kw)


CASES = {
    "banded6": _case(lambda: _banded(6, 33)),
    "banded7": _case(lambda: _banded(7, 33), na=7),
    "banded10": _case(lambda: _banded(10, 34), na=10),
    "mixed": _case(lambda: _ladybug(m=40, n=1500, max_track=30, radius=150.0, seed=23)),
    "long-140": _case(_long_edge),
    "points-unseen-single": _case(_unseen_single),
    "fix-motion": _case(lambda: _banded(6, 33), fix_motion=True),
    "fix-structure": _case(lambda: _banded(6, 33), pivot=False, fix_structure=True),
    "projective12-fix-structure": _case(lambda: _banded(12, 33), na=12, pivot=False,
                                        fix_structure=True, model="projective"),
    "banded6-ordered": _case(lambda: _banded(6, 33), ordered=1),
    "banded6-parity": _case(lambda: _banded(6, 33), parity=True),
}
LD_MAX = 400      # inverse_ld up to here, numpy.linalg.inv beyond


def _make(gpu, key):
    c = CASES[key]
    sc, pt, cam, ox = c["scene"]()
    na, kw = c["na"], dict(c["kw"])
    m, n = sc.m, sc.n
    if kw.get("model") == "projective":
        from bundleadjustmentmatlab_amd.scene import projective_from
        Pp, Xp = projective_from(sc)
        a, b = np.asfortranarray(Pp.reshape(12, m, order="F")), np.asfortranarray(Xp[0:3])
        K, kw["m"] = None, m
    else:
        (a, b), K = _params(sc, na), sc.K
    if c["pivot"]:
        kw["pivot"] = np.arange(m) < 2
    ba = gpu.BundleAdjuster(K, pt, cam, ox, n, na, **kw)
    return ba, dict(c, m=m, n=n, pt=pt, cam=cam, a=a, b=b)


_RUNS = {}


def _run(gpu, key):
    """One context per case, shared by the stages' tests and never modified."""
    if key in _RUNS:
        if isinstance(_RUNS[key], BaseException):    # never run a failed case again
            pytest.fail(f"{key}: the case's run failed in an earlier test: {_RUNS[key]!r}")
        return _RUNS[key]
    try:
        ba, r = _make(gpu, key)
        with ba:
            ba.set_params(r["a"], r["b"])
            r["lin"] = ba.linearization()
            r["red0"] = ba.reduced_system(dense=False)
            r["cov"] = ba.covariance(scale=False, full=True)
            r["red1"] = ba.reduced_system(dense=False)
            r["cov2"] = ba.covariance(scale=False, full=True)
            r["covs"] = ba.covariance(scale=True, full=True)
            r["info"] = ba.step(relinearize=False, update_lm=False)
        _RUNS[key] = r
    except BaseException as exc:
        _RUNS[key] = exc
        raise
    return r


_REFS = {}


def _camera_ref(r, key):
    """The camera stage's reference of a case (computed once): the long double
    S0 of the GPU's linearisation, its fixed rows, the reference inverse and
    the fp64 figures that set the bar."""
    if key in _REFS:
        return _REFS[key]
    L, na, m = r["lin"], r["na"], r["m"]
    Vi = sr.vinv_of(L["V"], 0.0)
    ref = sr.schur(m, r["n"], na, r["pt"], r["cam"], L["W"], L["V"], L["eB"], L["U"], L["eA"],
                   0.0, Vinv=Vi)
    S0 = cr.dense_lower(ref)
    fixed = cr.fixed_rows_of(S0)
    free = np.flatnonzero(~fixed)
    # the fp64 route that sets the bar: S0 formed in fp64, numpy.linalg.inv
    S64 = cr.schur_fp64(m, na, r["pt"], r["cam"], L["W"], Vi, L["U"])
    assert np.array_equal(np.diag(S64) == 0, fixed)
    inv64 = cr.inverse_fp64(S64, fixed)
    if na * m <= LD_MAX:
        want = cr.inverse_ld(S0, fixed)
    else:
        want = cr.inverse_fp64(sr.symmetrise(S0.astype(np.float64)), fixed)
    out = dict(Vi=Vi, fixed=fixed, want=want, inv64=inv64,
               floor_full=cr.block_figure(inv64, want, na),
               floor_diag=cr.block_figure(cr.diag_blocks(inv64, na), cr.diag_blocks(want, na), na),
               cond=np.linalg.cond(S64[np.ix_(free, free)]) if len(free) else 0.0)
    _REFS[key] = out
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_camera_stage(gpu, key):
    r = _run(gpu, key)
    ref, cov, na = _camera_ref(r, key), r["cov"], r["na"]
    full, fixed = cov["full"], ref["fixed"]
    fig_full = cr.block_figure(full, ref["want"], na)
    fig_diag = cr.block_figure(cov["cam"], cr.diag_blocks(ref["want"], na), na)
    print(f"COV camera {key}: ld {na * r['m']} fixed rows {int(fixed.sum())} cond(S0) "
          f"{ref['cond']:.2g}: diagonal blocks GPU {fig_diag:.3g} numpy {ref['floor_diag']:.3g}; "
          f"all blocks GPU {fig_full:.3g} numpy {ref['floor_full']:.3g}")
    assert np.array_equal(cov["cam"], cr.diag_blocks(full, na)), key
    assert np.array_equal(full, full.T), key
    assert np.all(full[fixed, :] == 0.0) and np.all(full[:, fixed] == 0.0), key
    assert cov["fixed_rows"] == int(fixed.sum()), key
    assert np.all(np.isfinite(full))
    assert cov["scratch_bytes"] == 8 * (na * r["m"]) ** 2
    assert fig_diag <= 8 * ref["floor_diag"] and fig_full <= 8 * ref["floor_full"], key


@pytest.mark.parametrize("key", list(CASES))
def test_point_stage(gpu, key):
    r = _run(gpu, key)
    na, L, cov = r["na"], r["lin"], r["cov"]
    Vi = sr.vinv_of(L["V"], 0.0)
    ref, bound = cr.point_cov(na, r["pt"], r["cam"], L["W"], Vi, cov["full"])
    ratio = cr.point_ratio(cov["pts"], ref, bound)
    track = np.bincount(r["pt"], minlength=r["n"])
    print(f"COV points {key}: {ratio:.3g} of the bound (longest track {track.max()}, "
          f"{int((track == 0).sum())} unseen)")
    pts = cov["pts"]
    assert np.array_equal(pts, pts.transpose(1, 0, 2)), key
    assert np.all(pts[:, :, track == 0] == 0.0), key
    if r["kw"].get("fix_structure"):
        assert np.all(pts == 0.0), key
    if r["kw"].get("fix_motion"):
        low = np.tril(np.ones((3, 3), dtype=bool))[:, :, None]
        assert np.array_equal(pts, np.where(low, Vi, Vi.transpose(1, 0, 2))), key
        assert np.all(cov["full"] == 0.0)
    assert np.all(np.isfinite(pts))
    assert ratio <= 1.0, (key, ratio)


@pytest.mark.parametrize("key", ["banded6", "banded10"])
def test_end_to_end(gpu, key):
    r = _run(gpu, key)
    ref, L, na, cov = _camera_ref(r, key), r["lin"], r["na"], r["cov"]
    pt, cam = r["pt"], r["cam"]
    seen = np.bincount(pt, minlength=r["n"]) > 0
    assert seen.all() and np.bincount(pt).min() >= 2
    full_a, full_b, _ = cr.normal_inverse(na, r["m"], r["n"], pt, cam, L["U"], L["V"], L["W"],
                                          ref["fixed"], seen)
    # the references' own two-route floor: the fp64 Schur route against it
    inv64 = ref["inv64"]
    b64 = cr.point_cov_fp64(na, pt, cam, L["W"], ref["Vi"], inv64)
    floor_a = cr.block_figure(inv64, full_a, na)
    floor_b = cr.block_figure(b64, full_b, 3)
    fig_a = cr.block_figure(cov["full"], full_a, na)
    fig_b = cr.block_figure(cov["pts"], full_b, 3)
    print(f"COV end-to-end {key}: cameras GPU {fig_a:.3g} floor {floor_a:.3g}; points GPU "
          f"{fig_b:.3g} floor {floor_b:.3g}")
    assert fig_a <= 8 * floor_a and fig_b <= 8 * floor_b, key


@pytest.mark.parametrize("key", list(CASES))
def test_call_leaves_the_state(gpu, key):
    """The reduced system at the context's lambda is the same before and after a
    call, two calls are bit-identical, scale is a multiplication by sigma2, and
    SSE / dof follow the definition."""
    r = _run(gpu, key)
    for x, y in zip(r["red0"], r["red1"]):
        assert np.array_equal(x, y), key
    cov, cov2, covs = r["cov"], r["cov2"], r["covs"]
    for k in ("cam", "pts", "full"):
        assert np.array_equal(cov[k], cov2[k]), (key, k)
        assert np.array_equal(covs[k], cov[k] * cov["sigma2"]), (key, k)
    for k in ("sse", "dof", "sigma2", "fixed_rows"):
        assert cov[k] == cov2[k] == covs[k], (key, k)
    fixed = _camera_ref(r, key)["fixed"]
    seen = int((np.bincount(r["pt"], minlength=r["n"]) > 0).sum())
    dof = 2 * len(r["pt"]) - ((~fixed).sum() + (0 if r["kw"].get("fix_structure") else 3 * seen))
    assert cov["sse"] == r["info"].old_sse, key
    assert cov["dof"] == dof and dof > 0, key
    assert cov["sigma2"] == cov["sse"] / dof, key
    print(f"COV state {key}: sse {cov['sse']:.6g} dof {dof} sigma2 {cov['sigma2']:.6g} "
          f"ms dense {cov['ms'][0]:.3f} points {cov['ms'][1]:.3f}")


@pytest.mark.parametrize("key", ["banded6", "banded6-ordered", "banded6-parity", "mixed",
                                 "long-140"])
def test_step_after_call_is_bit_identical(gpu, key):
    """step, covariance, step against step, step on a twin context; the last
    step read back after the call is the one before it."""
    out = []
    for with_cov in (True, False):
        ba, r = _make(gpu, key)
        with ba:
            ba.set_params(r["a"], r["b"])
            i1 = ba.step(relinearize=True, update_lm=True)
            s1 = [x.copy() for x in ba.last_step()]
            if with_cov:
                ba.covariance()
                for x, y in zip(s1, ba.last_step()):
                    assert np.array_equal(x, y), key
            i2 = ba.step(relinearize=True, update_lm=True)
            s2 = [x.copy() for x in ba.last_step()]
            i3 = ba.step(relinearize=False, update_lm=True)
            s3 = [x.copy() for x in ba.last_step()]
            p = ba.get_params()
        out.append(([i1, i2, i3], s1 + s2 + s3 + list(p)))
    (ia, xa), (ib, xb) = out
    for a, b in zip(ia, ib):
        for f, _ in a._fields_:
            assert getattr(a, f) == getattr(b, f), (key, f)
    assert ia[0].accepted == 1
    for a, b in zip(xa, xb):
        assert np.array_equal(a, b), key


@pytest.mark.parametrize("key", ["banded6", "banded7", "mixed", "long-140"])
def test_dense_and_packed_sources_agree(gpu, key, monkeypatch):
    """k_point_cov reads Sigma_a from the packed co-visible blocks (default) or
    straight from the dense inverse (VLGBA_COV_PACKED=0, read at a context's
    first call): the same values, so the same bits."""
    want = _run(gpu, key)["cov"]
    monkeypatch.setenv("VLGBA_COV_PACKED", "0")
    ba, r = _make(gpu, key)
    with ba:
        ba.set_params(r["a"], r["b"])
        cov = ba.covariance(scale=False)
    assert np.array_equal(cov["pts"], want["pts"]) and np.array_equal(cov["cam"], want["cam"])


def test_two_cameras_one_point(gpu):
    """Nothing is fixed and one point cannot pin two cameras: S0 is singular
    up to the forward differences' noise.  Whether dpotrf meets a non-positive
    pivot on it is decided by that noise, so the branch cannot be pinned more
    tightly than this: the call returns 0 with all-finite output, or
    VLGBA_E_SINGULAR, and nothing else."""
    sc, pt, cam, ox = _two_one()
    a, b = _params(sc, 6)
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 6) as ba:
        ba.set_params(a, b)
        try:
            cov = ba.covariance(scale=False, full=True)
        except gpu._lib.VlgbaError as exc:
            print(f"COV two-cameras-one-point: {exc}")
            assert "(-1007)" in str(exc)
        else:
            print(f"COV two-cameras-one-point: 0, largest |Sigma_a| "
                  f"{np.abs(cov['full']).max():.3g}")
            assert all(np.all(np.isfinite(cov[k])) for k in ("cam", "pts", "full"))
        info = ba.step()            # the context is still usable
        assert np.isfinite(info.new_sse)


def test_driver_return_covariance(gpu):
    """bundle_euclid_obs(return_covariance=True) appends the dict of a
    BundleAdjuster set to the returned parameters (after the stats)."""
    sc, pt, cam, ox = _banded(6, 33)
    opts = ("fix_calibration", "fix_pivot", [1, 2])
    out = gpu.bundle_euclid_obs(sc.K, sc.T0, sc.w0, sc.X0, pt, cam, ox, *opts,
                                return_stats=True, return_covariance=True)
    assert len(out) == 7 and hasattr(out[5], "iterations")
    K_, Te_, w_, Xe_, err, _, cov = out
    plain = gpu.bundle_euclid_obs(sc.K, sc.T0, sc.w0, sc.X0, pt, cam, ox, *opts)
    assert len(plain) == 5 and all(np.array_equal(x, y) for x, y in zip(plain, out[:5]))
    a = np.asfortranarray(np.vstack([w_, Te_]))
    with gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 6, pivot=np.arange(sc.m) < 2) as ba:
        ba.set_params(a, np.asfortranarray(Xe_[:3]))
        want = ba.covariance()
    for k in ("cam", "pts"):
        assert np.array_equal(cov[k], want[k]), k
    for k in ("sse", "dof", "sigma2", "fixed_rows", "scratch_bytes"):
        assert cov[k] == want[k], k
    assert sorted(cov) == sorted(want) and "full" not in cov
    assert cov["sse"] / len(pt) == pytest.approx(err[-1], rel=1e-12)
    assert np.all(cov["cam"][:, :, :2] == 0.0) and np.all(np.diagonal(cov["cam"][:, :, 2:]) > 0)
