"""The covariance reference (tests/cov_ref.py) proven on the CPU before it
judges the GPU (tests/test_gpu_covariance.py), and the binding's CPU facts.

Scene: the stage-reference scene (cfg2, m 33, n 1327, track 6, seed 41; num_a
6) linearised by the CPU oracle, first two cameras fixed; and num_a 10, m 34,
n 700, track 4.  Two independent fp64 routes to the covariance --
numpy.linalg.inv of the full normal matrix [[U, W], [W^T, V]], and
numpy.linalg.inv of the Schur complement formed in fp64 followed by the fp64
point formula -- differ by the "floor" (largest per-block max|diff| /
max|block| over the camera blocks and the point blocks).  The long double
Schur route (inverse_ld + point_cov) must sit inside that floor of the
full-matrix inverse.  Its distance to the full inverse is the full inverse's
own fp64 error (the long double route has none to speak of), which is one of
the two errors the floor is made of -- but the two fp64 routes' errors may
partly cancel in the floor, so the assertion allows the factor 8 that the GPU
tests allow between two fp64 algorithms: distance <= 8 x floor.

Measured (printed by the tests):
    num_a  6: floor 6.9e-10 (cameras 4.4e-10, points 6.9e-10), long double
              route 1.2e-09 from the full inverse (cameras 1.2e-09, points
              3.4e-10); cond(S0) 5.2e8
    num_a 10: floor 4.0e-07 (cameras 1.4e-07, points 4.0e-07), long double
              route 1.3e-08 (cameras 1.3e-08, points 1.1e-08); cond(S0) 2.5e12
    inverse_ld: |S0 Sigma_a - I| 9.7e-14 (an fp64 inverse: 3.3e-06);
    point_cov: an fp64 evaluation in numpy's order 0.029 of the bound
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import cov_ref as cr
import schur_ref as sr
from test_schur_ref import start_params, w_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {
    "banded6": (dict(m=33, n=1327, track=6, seed=41), 6),
    "banded10": (dict(m=34, n=700, track=4, seed=41), 10),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Computed once, shared, never modified."""
    import bundle_euclid_ref as oracle
    from bundleadjustmentmatlab_amd.scene import make_config
    kw, na = SCENES[name]
    sc = make_config("cfg2", **kw)
    a, b = start_params(sc, na)
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    L = oracle.sp_linearize(pb, a, b, na)
    L = dict(L, W=w_of(L["W"], na))
    L = cr.apply_pivot(L, sc.obs_cam, np.arange(sc.m) < 2)
    m, n, pt, cam = sc.m, sc.n, sc.obs_pt, sc.obs_cam
    Vi = sr.vinv_of(L["V"], 0.0)
    ref = sr.schur(m, n, na, pt, cam, L["W"], L["V"], L["eB"], L["U"], L["eA"], 0.0, Vinv=Vi)
    S0 = cr.dense_lower(ref)
    fixed = cr.fixed_rows_of(S0)
    seen = np.bincount(pt, minlength=n) > 0
    # long double Schur route
    cov_a = cr.inverse_ld(S0, fixed)
    cov_a64 = cov_a.astype(np.float64)
    cov_b, bound = cr.point_cov(na, pt, cam, L["W"], Vi, cov_a64)
    # fp64 Schur route: S0 formed in fp64, numpy.linalg.inv, the fp64 point formula
    S64 = cr.schur_fp64(m, na, pt, cam, L["W"], Vi, L["U"])
    free = np.flatnonzero(~fixed)
    inv64 = cr.inverse_fp64(S64, fixed)
    cov_b64 = cr.point_cov_fp64(na, pt, cam, L["W"], Vi, inv64)
    # fp64 full normal matrix
    full_a, full_b, H = cr.normal_inverse(na, m, n, pt, cam, L["U"], L["V"], L["W"], fixed, seen)
    return dict(sc=sc, na=na, L=L, Vi=Vi, S0=S0, fixed=fixed, cov_a=cov_a, cov_a64=cov_a64,
                cov_b=cov_b, bound=bound, inv64=inv64, cov_b64=cov_b64, full_a=full_a,
                full_b=full_b, cond_s=np.linalg.cond(S64[np.ix_(free, free)]))


@pytest.mark.parametrize("name", list(SCENES))
def test_reference_inside_the_two_route_floor(oracle, name):
    c = _case(name)
    na = c["na"]
    assert c["fixed"].sum() == 2 * na and np.all(c["fixed"][:2 * na])
    floor_a = cr.block_figure(c["inv64"], c["full_a"], na)
    floor_b = cr.block_figure(c["cov_b64"], c["full_b"], 3)
    ref_a = cr.block_figure(c["full_a"], c["cov_a"], na)
    ref_b = cr.block_figure(c["full_b"], c["cov_b"], 3)
    floor, ref = max(floor_a, floor_b), max(ref_a, ref_b)
    print(f"COV-REF {name}: two fp64 routes differ by {floor:.2g} (cameras {floor_a:.2g}, "
          f"points {floor_b:.2g}); long double Schur route vs the full inverse {ref:.2g} "
          f"(cameras {ref_a:.2g}, points {ref_b:.2g}); cond(S0) {c['cond_s']:.2g}")
    assert ref <= 8 * floor
    # fixed rows and columns are exactly zero, the matrix exactly symmetric
    assert np.all(c["cov_a"][c["fixed"], :] == 0) and np.all(c["cov_a"][:, c["fixed"]] == 0)
    assert np.array_equal(c["cov_a"], c["cov_a"].T)


def test_inverse_ld_residual(oracle):
    """S0 Sigma_a = I on the free rows to long double accuracy: cond(S0) times
    a few hundred roundings of 2^-64 -- four orders below what an fp64 inverse
    of the same matrix leaves."""
    c = _case("banded6")
    free = ~c["fixed"]
    S = (np.tril(c["S0"]) + np.tril(c["S0"], -1).T)[np.ix_(free, free)]
    eye = np.eye(S.shape[0], dtype=sr.LD)
    res = float(np.abs(S @ c["cov_a"][np.ix_(free, free)] - eye).max())
    res64 = float(np.abs(S @ c["inv64"][np.ix_(free, free)].astype(sr.LD) - eye).max())
    bar = float(S.shape[0] * c["cond_s"] * 2.0 ** -64)
    print(f"COV-REF inverse_ld: |S Sigma - I| {res:.2g} (bar {bar:.2g}); fp64 inverse {res64:.2g}")
    assert res <= bar
    assert res64 > 100 * res
    with pytest.raises(np.linalg.LinAlgError):
        cr.inverse_ld(-np.eye(3), np.zeros(3, bool))
    inv = cr.inverse_ld(np.diag([2.0, 0.0, 4.0]), np.array([False, True, False]))
    assert np.array_equal(inv.astype(float), np.diag([0.5, 0.0, 0.25]))


def test_point_bound_holds_and_has_teeth(oracle):
    c = _case("banded6")
    na, sc, L = c["na"], c["sc"], c["L"]
    # an fp64 evaluation in another order (all ordered pairs, numpy's sums)
    got = cr.point_cov_fp64(na, sc.obs_pt, sc.obs_cam, L["W"], c["Vi"], c["cov_a64"])
    got = np.tril(got.transpose(2, 0, 1)) + np.tril(got.transpose(2, 0, 1), -1).transpose(0, 2, 1)
    got = got.transpose(1, 2, 0)
    r = cr.point_ratio(got, c["cov_b"], c["bound"])
    print(f"COV-REF point_cov: fp64 in numpy's order {r:.3g} of the bound")
    assert r <= 1.0
    # one entry off by 1e-10 relative: the best-determined one (on this scene
    # cond(S0) = 5e8 and the correction V+ T V+ cancels heavily: the median
    # bound is 2e-9 of its entry, the smallest 3e-14)
    rel = (c["bound"] / np.abs(c["cov_b"])).astype(float)
    q = np.unravel_index(np.argmin(rel), rel.shape)
    assert rel[q] < 1e-12
    bad = got.copy()
    bad[q] *= 1 + 1e-10
    assert cr.point_ratio(bad, c["cov_b"], c["bound"]) > 1.0
    # one pair's term dropped / the pivot cameras' columns not zeroed / V+ alone
    i = int(sc.obs_pt[len(sc.obs_pt) // 2])
    o = np.flatnonzero(sc.obs_pt == i)
    j, k = sc.obs_cam[o[-1]], sc.obs_cam[o[0]]
    M = L["W"][:, :, o[-1]].T @ c["cov_a64"][na * j:na * j + na, na * k:na * k + na] \
        @ L["W"][:, :, o[0]]
    bad = got.copy()
    bad[:, :, i] -= c["Vi"][:, :, i] @ (M + M.T) @ c["Vi"][:, :, i]
    assert cr.point_ratio(bad, c["cov_b"], c["bound"]) > 1.0
    assert cr.point_ratio(c["Vi"], c["cov_b"], c["bound"]) > 1.0
    # exact zeros where the bound is zero
    Vz = c["Vi"].copy()
    Vz[:, :, :5] = 0.0
    ref, bound = cr.point_cov(na, sc.obs_pt, sc.obs_cam, L["W"], Vz, c["cov_a64"])
    assert np.all(ref[:, :, :5] == 0) and np.all(bound[:, :, :5] == 0)
    tiny = np.zeros_like(got)
    tiny[0, 0, 0] = 1e-300
    assert cr.point_ratio(np.asarray(ref, float) + tiny, ref, bound) == np.inf
    assert np.array_equal(cr.chain_length(6, [0, 1, 6, 140]), [25, 26, 28, 1259])


def test_binding_declares_covariance():
    """The header and the library agree on the new entry point (ABI 6)."""
    from bundleadjustmentmatlab_amd import _lib
    with open(os.path.join(ROOT, "include", "vlgba.h")) as f:
        hdr = f.read()
    assert "#define VLGBA_E_SINGULAR (-1007)" in hdr
    assert "int vlgba_covariance(vlgba_ctx *ctx, int scale, double *cov_a, double *cov_a_full," in hdr
    assert _lib.ABI_VERSION == 6 and "#define VLGBA_ABI_VERSION 6" in hdr
    assert -1007 in _lib.ERRORS
    L = _lib.lib()
    assert L.vlgba_covariance.argtypes == [ctypes.c_void_p, ctypes.c_int] + [_lib.c_dp] * 4
    assert L.vlgba_covariance(None, 1, None, None, None, None) == -1001
