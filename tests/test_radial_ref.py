"""tests/radial_ref.py -- the reference of the radial-distortion camera (num_a =
9) -- proved on the CPU before tests/test_gpu_radial.py holds the kernels to it.

1. The closed-form Jacobian against long double central differences of the true
   projection, step 1e-5 (truncation h^2 / 6 times the third derivative,
   cancellation 2^-64 |x| / h ~ 1e-12 px), at jac_ref's bar: 1e-9 of the row's
   largest entry.  The coefficient columns are linear in k1, k2: exact there.
2. At k1 = k2 = 0 the projection, so the residuals, are jac_ref's num_a = 7
   ones (a few long double roundings: the order of f d u against f Xc_0 / Xc_2).
3. The bounds' caps: a Jacobian entry's at most 1e-12 of the largest |entry| of
   the observation's [A | B] (jac_ref's cap), a projection's at most 1e-12 of
   the largest |coordinate| of the image (about 45 roundings along its chain,
   5e-15, times the cancellation of R b + T, which the bound pays for where it
   happens: the same allowance of 200 as jac_ref's cap makes).
4. An fp64 evaluation of the same formulas in numpy (another order of the sums)
   lies within the bounds of project, jacobians and linearization: the bounds
   do cover an fp64 evaluation, and linearization() propagates them.
5. radial_lm recovers the planted coefficients on the end-to-end scene.
6. bundle_euclid(..., radial=kd0) packs a = [w; T; f; k1; k2] and unpacks the
   refined coefficients as an extra last output; every other call is unchanged.
7. include/vlgba.h still says ABI 6 and describes the model.
"""
import functools
import os
import re

import numpy as np

import jac_ref as jr
import radial_ref as ra
import robust_ref as rr
from conftest import random_problem

LD = ra.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _problem(seed=3):
    """conftest's random num_a = 7 problem (camera 0 at w = 0) with coefficients
    near ra.K_TRUE per camera: (K, a7, a9, b, pt, cam, obs_x)."""
    K, a7, b, X, vis, _ = random_problem(seed, num_a=7, zero_w_cam=True)
    rng = np.random.default_rng(seed + 50)
    m = a7.shape[1]
    kd = np.array(ra.K_TRUE)[:, None] * rng.uniform(0.7, 1.3, (2, m))
    a9 = np.asfortranarray(np.vstack([a7, kd]))
    pt, cam = np.nonzero(vis)
    return K, a7, a9, b, pt, cam, np.ascontiguousarray(X[:, pt, cam].T)


def test_against_long_double_central_differences():
    K, _, a, b, pt, cam, _ = _problem()
    Ao, Bo, _, _ = ra.jacobians(K, a, b, pt, cam)
    Acd, Bcd = ra.central_differences(K, a, b, pt, cam, 1e-5)
    scale = jr.row_max(Ao, Bo)
    dA = (np.abs(Ao - Acd).reshape(len(pt), -1).max(1) / scale).max()
    dB = (np.abs(Bo - Bcd).reshape(len(pt), -1).max(1) / scale).max()
    lin = (np.abs(Ao - Acd)[:, :, 7:9].reshape(len(pt), -1).max(1) / scale).max()
    print(f"RADIAL central differences: A {float(dA):.2e} B {float(dB):.2e} of the row's "
          f"largest entry (coefficient columns {float(lin):.2e})")
    assert np.all(Ao[:, :, 6:9] != 0) and dA <= 1e-9 and dB <= 1e-9, (dA, dB)
    # no truncation there, only the differences' cancellation: 2 roundings of |x| over 2 h
    xmax = np.abs(ra.project_true(K, a, b, pt, cam)).max()
    assert lin <= 4 * LD(2.0) ** -64 * xmax / LD(1e-5) / scale.min(), (lin, xmax, scale.min())


def test_zero_coefficients_give_the_num_a_7_residuals():
    K, a7, a9, b, pt, cam, ox = _problem()
    a0 = a9.copy()
    a0[7:9] = 0.0
    x9 = ra.project_true(K, a0, b, pt, cam)
    x7 = jr.project(K, a7, b, pt, cam, 7)
    d = np.abs(x9 - x7).max()
    cap = 8 * LD(2.0) ** -63 * np.abs(x7).max()
    # ... and the kernel-order evaluation is the same projection (camera 0: R = I both ways)
    xk, xb = ra.project(K, a0, b, pt, cam)
    print(f"RADIAL k = 0: largest |x9 - x7| {float(d):.2e} (cap {float(cap):.2e}); kernel order "
          f"against the true projection {float((np.abs(xk - x9) / xb).max()):.3g} of its bound")
    assert d <= cap
    assert np.all(np.abs(xk - x9) <= xb)
    e9 = ra.residuals(K, a0, b, pt, cam, ox)[0]
    assert np.abs(e9 - (ox.astype(LD) - x7)).max() <= cap + xb.max()
    assert np.abs(ra.project_true(K, a9, b, pt, cam) - x7).max() > 1e-3     # the lens does bite


def test_bounds_are_capped():
    K, _, a, b, pt, cam, _ = _problem()
    Ao, Bo, Ab, Bb = ra.jacobians(K, a, b, pt, cam)
    rel = np.maximum(Ab.reshape(len(pt), -1).max(1), Bb.reshape(len(pt), -1).max(1)) \
        / jr.row_max(Ao, Bo)
    x, xb = ra.project(K, a, b, pt, cam)
    prel = xb.max() / np.abs(x).max()
    print(f"RADIAL caps: Jacobian bound {float(rel.max()):.2e} of the row's largest entry, "
          f"projection bound {float(prel / ra.U53):.1f} u of the largest coordinate")
    assert np.all(Ab >= 0) and np.all(Bb >= 0) and rel.max() <= 1e-12
    assert prel <= 1e-12


def _fp64(K, a, b, pt, cam):
    """The model in plain numpy fp64 (sums in numpy's order, n n' formed as a
    matrix): x (N, 2), A (N, 2, 9), B (N, 2, 3)."""
    R = np.asarray(jr.table_rotation(a[0:3])[0], dtype=np.float64)[:, :, cam]
    D = np.asarray(jr.drodrigues(a[0:3])[0], dtype=np.float64)[:, :, :, cam]
    bo = b[:, pt]
    Xc = np.einsum("ijo,jo->io", R, bo) + a[3:6, cam]
    n = Xc[0:2] / Xc[2]
    r2 = (n * n).sum(0)
    f, k1, k2 = a[6, cam], a[7, cam], a[8, cam]
    d = 1 + k1 * r2 + k2 * r2 * r2
    x = (f * d * n + K[2:4, cam]).T
    g = 2 * k1 + 4 * k2 * r2
    Jn = f * (d * np.eye(2)[:, :, None] + g * n[:, None, :] * n[None, :, :])      # (2, 2, N)
    P = np.zeros((2, 3, len(pt)))
    P[0, 0] = P[1, 1] = 1 / Xc[2]
    P[:, 2] = -n / Xc[2]
    Jx = np.einsum("ijo,jko->iko", Jn, P)
    A = np.zeros((len(pt), 2, 9))
    A[:, :, 0:3] = np.einsum("ijo,jko->oik", Jx, np.einsum("ijko,jo->iko", D, bo))
    A[:, :, 3:6] = Jx.transpose(2, 0, 1)
    A[:, :, 6] = (d * n).T
    A[:, :, 7] = (f * r2 * n).T
    A[:, :, 8] = (f * r2 * r2 * n).T
    B = np.einsum("ijo,jko->oik", Jx, R)
    return x, A, B


def test_an_fp64_evaluation_lies_within_the_bounds():
    K, _, a, b, pt, cam, ox = _problem()
    m, n = a.shape[1], b.shape[1]
    x64, A64, B64 = _fp64(K, a, b, pt, cam)
    x, xb = ra.project(K, a, b, pt, cam)
    Ao, Bo, Ab, Bb = ra.jacobians(K, a, b, pt, cam)
    fig = dict(x=rr.ratio(x64, x, xb), A=rr.ratio(A64, Ao, Ab), B=rr.ratio(B64, Bo, Bb))
    e64 = ox - x64
    e, eb = ra.residuals(K, a, b, pt, cam, ox)
    fig["e"] = rr.ratio(e64, e, eb)
    c, cb = ra.cost(K, a, b, pt, cam, ox)
    fig["cost"] = rr.ratio(float((e64 * e64).sum()), c, cb)
    # the sums of the fp64 rows, in numpy's order, against linearization()
    pivot = np.arange(m) < 1
    R = ra.linearization(K, a, b, pt, cam, e64, m, n, pivot=pivot)
    W = np.einsum("okr,okc->rco", A64, B64)
    W[:, :, pivot[cam]] = 0
    U, V = np.zeros((9, 9, m)), np.zeros((3, 3, n))
    eA, eB = np.zeros((9, m)), np.zeros((3, n))
    for o in range(len(pt)):
        V[:, :, pt[o]] += B64[o].T @ B64[o]
        eB[:, pt[o]] += B64[o].T @ e64[o]
        if not pivot[cam[o]]:
            U[:, :, cam[o]] += A64[o].T @ A64[o]
            eA[:, cam[o]] += A64[o].T @ e64[o]
    got = dict(U=U, eA=eA, V=V, eB=eB, W=W)
    for k in got:
        fig[k] = rr.ratio(got[k], R[k], R[k + "_b"])
    print("RADIAL fp64 evaluation, largest |diff| / bound: "
          + " ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert all(v <= 1.0 for v in fig.values()), fig
    assert np.all(R["U_b"][:, :, 0] == 0) and np.all(R["U_b"][:, :, 1:] > 0)
    # the propagated part is there: the bounds exceed the sums' own
    Ao64 = np.asarray(Ao, dtype=np.float64)
    plain = rr.weighted(m, n, 9, pt, cam, Ao64, np.asarray(Bo, dtype=np.float64), e64, "none",
                        1.0, pivot=pivot)
    assert np.all(R["W_b"] >= plain["W_b"]) and np.any(R["W_b"] > plain["W_b"])


def test_radial_lm_recovers_the_coefficients():
    s = ra.e2e_scene()
    free = ~s["pivot"]
    a, b, err = ra.radial_lm(s["K"], s["a0"], s["b0"], s["pt"], s["cam"], s["obs_x"],
                             pivot=s["pivot"], **ra.E2E["stop"])
    dk = np.abs(a[7:9] - s["a_true"][7:9])[:, free].max(1)
    print(f"RADIAL cpu lm: error_ {err[0]:.6g} -> {err[-1]:.10g} in {len(err)} accepted steps; "
          f"k1 {a[7, free].min():.4f} .. {a[7, free].max():.4f} (truth {ra.K_TRUE[0]}), k2 "
          f"{a[8, free].min():.4f} .. {a[8, free].max():.4f} (truth {ra.K_TRUE[1]})")
    assert np.all(np.diff(err) < 0) and len(err) >= 4
    # an exact fit's noise floor is 2 sigma^2 = 0.5 px^2; the pivots stay put
    assert err[-1] < 1.0 < err[0]
    assert np.array_equal(a[:, s["pivot"]], s["a0"][:, s["pivot"]])
    # k1 to a third of its size: the start (0) is not within that
    assert dk[0] <= abs(ra.K_TRUE[0]) / 3, dk


class _FakeAdjuster:
    """Stands in for BundleAdjuster: records what it is given, returns it moved."""
    last = None

    def __init__(self, K, obs_pt, obs_cam, obs_x, n, num_a, **kw):
        self.num_a, self.kw, self.m = num_a, kw, np.shape(K)[1]
        _FakeAdjuster.last = self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def get_jacobian(self):
        return "analytic" if self.num_a == 9 else "fd"

    def set_params(self, a, b):
        self.a, self.b = np.array(a), np.array(b)

    def run(self):
        return np.array([2.0, 1.0]), "stats"

    def get_params(self):
        return self.a + 1.0, self.b + 1.0


def test_radial_packs_and_unpacks(monkeypatch):
    from bundleadjustmentmatlab_amd import bundle
    monkeypatch.setattr(bundle, "BundleAdjuster", _FakeAdjuster)
    m, n = 3, 4
    rng = np.random.default_rng(0)
    K = rng.uniform(500, 600, (4, m))
    Te, w = rng.standard_normal((3, m)), rng.standard_normal((3, m))
    Xe = np.vstack([rng.standard_normal((3, n)), 2 * np.ones((1, n))])
    x = rng.uniform(1, 2, (3, n, m))
    kd0 = rng.standard_normal((2, m))
    for fn, x4 in ((bundle.bundle_euclid, 2.0), (bundle.bundle_euclid_nomex, 1.0)):
        out = fn(K, Te, w, Xe, x, "fix_calibration", radial=kd0)
        fake = _FakeAdjuster.last
        assert fake.num_a == 9 and len(out) == 6
        assert np.array_equal(fake.a, np.vstack([w, Te, K[0:1], kd0]))
        assert np.array_equal(fake.b, Xe[0:3])
        K_, Te_, w_, Xe_, err, kd = out
        assert np.array_equal(kd, kd0 + 1.0) and kd.shape == (2, m)
        assert np.array_equal(K_[0], K[0] + 1.0) and np.array_equal(K_[1], K[0] + 1.0)
        assert np.array_equal(K_[2:4], K[2:4])                       # the principal point stays
        assert np.array_equal(Te_, Te + 1.0) and np.array_equal(w_, w + 1.0)
        assert np.array_equal(Xe_, np.vstack([Xe[0:3] + 1.0, x4 * np.ones((1, n))]))
        st = fn(K, Te, w, Xe, x, radial=kd0, return_stats=True)
        assert len(st) == 7 and st[5] == "stats" and np.array_equal(st[6], kd0 + 1.0)
    # without radial=: what it returned before
    for opts, na in ((("fix_calibration",), 6), (("fix_principal",), 7), ((), 10)):
        out = bundle.bundle_euclid(K, Te, w, Xe, x, *opts)
        assert _FakeAdjuster.last.num_a == na and len(out) == 5
    try:
        bundle.bundle_euclid(K, Te, w, Xe, x, radial=kd0[:, :2])
    except ValueError:
        pass
    else:
        raise AssertionError("a 2 x (m - 1) radial= was accepted")
    try:
        bundle.bundle_euclid(K, Te, w, Xe, x, radial=kd0, jacobian="fd")
    except ValueError:
        pass
    else:
        raise AssertionError("radial= with jacobian='fd' was accepted")


def test_header_says_abi_6_and_describes_the_model():
    h = open(os.path.join(ROOT, "include", "vlgba.h"), encoding="utf-8").read()
    assert re.search(r"#define\s+VLGBA_ABI_VERSION\s+6\b", h)
    from bundleadjustmentmatlab_amd import _lib
    assert _lib.ABI_VERSION == 6
    assert re.search(r"num_a\s*=?\s*9", h) and "k1" in h and "k2" in h
