"""The batched one-block entries' shared code on the CPU (tests/native/
block_host.cpp, g++ with no HIP include path): the LM driver of
csrc/ba_batch_lm.h, the per-point pass of csrc/ba_triang_math.h that
k_intersect_pass runs, and the NA x NA solve of csrc/ba_small_solve.h that
k_resect_pass runs on lane 0.  No GPU.

* The driver on a CPU backend around the per-point pass returns error_ and X
  bit for bit equal to the oracle's one-point bundle_euclid on the batches of
  tests/test_gpu_intersect.py (113 and 31 problems, both option sets).
* The pass with a mode of "no lens, FD, no loss" returns the bits of the
  mode-less instantiation; tri_point<true> with a lens of zeros agrees with
  tri_point<false> to the bar of tests/test_gpu_block_model.py (equal status,
  1e-9 relative).
* The solve at NA 6 / 7 / 9 / 10: oracle.chol_seq's bits on positive definite
  input; the zero-row rule; and the cyclic-Jacobi pinv(S) e_ on indefinite
  input within 8 x the error of LAPACK's (oracle.matlab_pinv) against a
  50-digit mpmath eigendecomposition with the same cut, each the largest over
  20 inputs.  Measured (largest relative error of da / of LAPACK's / largest
  ratio of the two on one input): NA 6 5.7e-14 / 4.2e-13 / 9.00, NA 7
  9.5e-14 / 7.8e-14 / 3.47, NA 9 6.7e-14 / 5.2e-14 / 3.54, NA 10 6.6e-14 /
  6.0e-14 / 11.04.
* The driver's bookkeeping on a stub backend that reports a script.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_intersect as gi
import triang_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_lp = ctypes.POINTER(ctypes.c_longlong)


def _P(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def bh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bh") / "libbh.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                    os.path.join(HERE, "native", "block_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.bh_intersect.argtypes = [ctypes.c_int, _dp, _dp, _dp, ctypes.c_longlong, _lp, _ip, _dp,
                               ctypes.c_void_p, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_int,
                               ctypes.c_double, _dp, _dp, ctypes.c_int, _ip, ctypes.c_void_p]
    L.bh_triangulate.argtypes = [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_longlong, _lp, _ip,
                                 _dp, _dp, _ip]
    L.bh_triangulate.restype = None
    L.bh_small_solve.argtypes = [ctypes.c_int, _dp, ctypes.c_double, _dp]
    L.bh_scripted.argtypes = [ctypes.c_int, _lp, ctypes.c_void_p, ctypes.c_int, _dp, _dp, _dp,
                              ctypes.c_int, _ip, ctypes.c_void_p]
    return L


def _options(**kw):
    from bundleadjustmentmatlab_amd._lib import VlgbaOptions
    opt = VlgbaOptions()
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt, (kw.get("max_iter", 0) or 20) + 1


def _csr(sc, cl, xl):
    K, T, w = (np.asfortranarray(q, dtype=np.float64) for q in (sc.K, sc.T, sc.w))
    ptr, cam, x = tr.pack(cl, xl)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    cam = np.ascontiguousarray(cam, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
    return K, T, w, ptr, cam, x


def _intersect(bh, sc, cl, xl, X0, mode, **kw):
    """bh_intersect -> (X_ (4 x n), errs, stats)"""
    from bundleadjustmentmatlab_amd._lib import VlgbaStats
    K, T, w, ptr, cam, x = _csr(sc, cl, xl)
    n = len(ptr) - 1
    opt, cap = _options(**kw)
    b = np.ascontiguousarray(X0[:3].T).reshape(-1)
    err, nerr, st = np.zeros((n, cap)), np.zeros(n, dtype=np.int32), VlgbaStats()
    rc = bh.bh_intersect(sc.m, _P(K), _P(T), _P(w), n, ptr.ctypes.data_as(_lp),
                         cam.ctypes.data_as(_ip), _P(x), ctypes.addressof(opt), mode, None, 0, 0,
                         0.0, _P(b), _P(err), cap, nerr.ctypes.data_as(_ip),
                         ctypes.addressof(st))
    assert rc == 0
    X_ = np.array(X0, order="F")
    X_[:3] = b.reshape(n, 3).T
    return X_, [err[q, :nerr[q]].copy() for q in range(n)], st


@pytest.mark.parametrize("kw", [{}, {"lambda0": 1e-2, "max_iter": 3}],
                         ids=["defaults", "lambda0-max_iter"])
@pytest.mark.parametrize("which", ["short", "long"])
def test_host_intersect_bit_identical_to_the_oracle(bh, oracle, which, kw):
    sc, cl, xl, X0, ref = gi._reference(oracle, which, kw)
    assert len(cl) == (113 if which == "short" else 31)
    X_, errs, st = _intersect(bh, sc, cl, xl, X0, -1, **kw)
    for q, (Xr, er) in enumerate(ref):
        assert np.array_equal(errs[q], er), (q, len(cl[q]), errs[q], er)
        assert np.array_equal(X_[:, q], Xr), (q, X_[:, q] - Xr)
    assert st.accepted == sum(len(er) - 1 for _, er in ref if len(er))
    assert st.iterations >= st.accepted and st.pinv_passes == 0


def test_mode_of_nothing_folds_to_the_plain_pass(bh):
    sc, cl, xl, X0 = gi._batch_short()
    X0_, e0, s0 = _intersect(bh, sc, cl, xl, X0, -1)
    X1_, e1, s1 = _intersect(bh, sc, cl, xl, X0, 0)
    assert np.array_equal(X0_, X1_) and (s0.iterations, s0.accepted) == (s1.iterations, s1.accepted)
    assert len(e0) == len(e1) and all(np.array_equal(p, q) for p, q in zip(e0, e1))


def test_lens_of_zeros_agrees_with_the_plain_triangulation(bh):
    sc, cl, xl, _ = gi._batch_short()
    K, T, w, ptr, cam, x = _csr(sc, cl, xl)
    K[1] = K[0]                       # under a lens f = K[0] serves both axes
    n = len(ptr) - 1
    out = []
    for kd in (None, np.zeros((sc.m, 2))):
        X, st = np.zeros((4, n), order="F"), np.zeros(n, dtype=np.int32)
        bh.bh_triangulate(sc.m, _P(K), _P(T), _P(w), None if kd is None else _P(kd), n,
                          ptr.ctypes.data_as(_lp), cam.ctypes.data_as(_ip), _P(x), _P(X),
                          st.ctypes.data_as(_ip))
        out.append((X, st))
    (X0, s0), (Xz, sz) = out
    assert np.array_equal(s0, sz) and (s0 == 1).sum() >= 100
    ok = s0 == 1
    rel = tr.rel_err(Xz[:, ok], X0[:, ok])
    print(f"zero lens against plain: {rel:.3e} over {ok.sum()} points")
    assert rel <= 1e-9


# ---- the NA x NA solve -------------------------------------------------------
NAS = [6, 7, 9, 10]


def _solve(bh, na, S, rhs, lam=0.0):
    """bh_small_solve on st = S (column major) | rhs -> (da, fallback flag)"""
    st = np.concatenate([np.asarray(S).reshape(-1, order="F"), rhs]).astype(np.float64)
    da = np.full(na, np.nan)
    flag = bh.bh_small_solve(na, _P(st), lam, _P(da))
    return da, flag


def _spd(na, seed):
    rng = np.random.default_rng(1000 * na + seed)
    A = rng.standard_normal((12, na))
    U = A.T @ A
    U = np.tril(U) + np.tril(U, -1).T
    return U, rng.standard_normal(na)


def _damped(U, lam):
    S = U.copy()
    for k in range(len(S)):
        S[k, k] = (1 + lam) * U[k, k]
    return S


@pytest.mark.parametrize("na", NAS)
def test_solve_is_the_sequential_cholesky(bh, oracle, na):
    for seed in range(20):
        U, rhs = _spd(na, seed)
        da, flag = _solve(bh, na, U, rhs, 1e-3)
        want, rc = oracle.chol_seq(_damped(U, 1e-3), rhs)
        assert rc == 0 and flag == 0 and np.array_equal(da, want[:, 0]), (seed, da - want[:, 0])


@pytest.mark.parametrize("na", NAS)
def test_solve_zero_row_rule(bh, oracle, na):
    for seed in range(20):
        U, rhs = _spd(na, seed)
        k = seed % na
        U[k, :] = 0.0
        U[:, k] = 0.0
        da, flag = _solve(bh, na, U, rhs, 1e-3)
        S, e_ = _damped(U, 1e-3), rhs.copy()
        S[k, k], e_[k] = 1.0, 0.0
        want, rc = oracle.chol_seq(S, e_)
        assert rc == 0 and flag == 0 and da[k] == 0.0 and rhs[k] != 0.0
        assert np.array_equal(da, want[:, 0]), (seed, k)


def _indefinite(na, seed):
    """S = Q diag(d) Q': one negative eigenvalue, one of at most 1e-18 max |d|,
    the rest in [1e-3, 1] max |d|"""
    rng = np.random.default_rng(7000 * na + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((na, na)))
    top = 10.0 ** rng.uniform(-2, 2)
    d = top * 10.0 ** rng.uniform(-3, 0, na)
    d[rng.integers(na)] = top
    i, j = rng.choice(na, 2, replace=False)
    d[i] = -d[i]
    d[j] = 1e-18 * top * rng.uniform(0, 1)
    S = (Q * d) @ Q.T
    return np.tril(S) + np.tril(S, -1).T, rng.standard_normal(na)


def _pinv_mp(S, rhs):
    """pinv(S) rhs from a 50-digit eigendecomposition, MATLAB's cut
    NA * eps(max |eigenvalue|)"""
    import mpmath as mp
    with mp.workdps(50):
        na = len(S)
        ev, V = mp.eigsy(mp.matrix(S.tolist()))
        top = max(abs(e) for e in ev)
        tol = na * mp.mpf(float(np.spacing(float(top))))
        x = mp.matrix(na, 1)
        r = mp.matrix(rhs.tolist())
        kept = 0
        for k in range(na):
            if abs(ev[k]) > tol:
                kept += 1
                x += V[:, k] * ((V[:, k].T * r)[0] / ev[k])
        # away from the cut (the rounding of S itself moves the planted 1e-18
        # to about 1e-17 .. 1e-16 of the largest): nothing within a factor 4
        assert all(abs(e) > 4 * tol or abs(e) < tol / 4 for e in ev)
        return np.array([float(v) for v in x]), kept, x


@pytest.mark.parametrize("na", NAS)
def test_solve_jacobi_pinv(bh, oracle, na):
    """The error of the LAPACK reference is its largest over the 20 inputs, as
    the batch maxima of tests/test_gpu_triangulate.py: on one input it scatters
    over two decades (7.6e-16 .. 4.2e-13 here, both methods at or below the order
    of the condition 1e3 times the unit roundoff), so a ratio on one input says little
    -- it reaches 11 where LAPACK's own error happens to be 1e-15.  The module
    docstring has the measured figures."""
    import mpmath as mp
    worst = [0.0, 0.0, 0.0]
    for seed in range(20):
        S, rhs = _indefinite(na, seed)
        da, flag = _solve(bh, na, S, rhs)
        assert flag == 1
        _, kept, xm = _pinv_mp(S, rhs)
        assert kept == na - 1
        with mp.workdps(50):     # errors against the 50-digit vector itself
            def rel(v):
                return float(mp.norm(mp.matrix(v.tolist()) - xm) / mp.norm(xm))
            e_da, e_lapack = rel(da), rel(oracle.matlab_pinv(S) @ rhs)
        print(f"NA {na} seed {seed}: jacobi {e_da:.3e}  lapack {e_lapack:.3e}  "
              f"ratio {e_da / e_lapack:.2f}")
        worst = [max(p, q) for p, q in zip(worst, (e_da, e_lapack, e_da / e_lapack))]
    print(f"NA {na}: largest jacobi {worst[0]:.3e}  lapack {worst[1]:.3e}  "
          f"largest ratio on one input {worst[2]:.2f}")
    assert worst[0] <= 8 * worst[1]


# ---- the driver's bookkeeping ---------------------------------------------------
def test_driver_bookkeeping_on_a_scripted_backend(bh):
    """3 problems of 2 / 4 / 5 observations, max_iter 5, max_iter2 2, every
    pass's (old, new, dpg, flag) scripted; by hand from bundle_euclid.m:218-241
    (and :120-123 for who goes on):
      problem 0: accepted (8 -> 2), rejected, rejected (flag 1): iter2 = 2 stops
                 it; error_ = [4, 1]; lambda 1e-3 * 1/3 * 2 * 4
      problem 1: accepted 16 -> 8, 8 -> 4 (flag 1), 4 -> 3.999, then the drop
                 1 - 0.99975 is not above 1e-3 * 1: error_ = [4, 2, 1, 0.99975]
      problem 2: accepted four times (the last with flag 1), then iter = 5 =
                 max_iter: error_ = [2, 1, 0.5, 0.25, 0.1]
    In pass 4 only problem 2 runs; problem 0's flag of pass 3 still stands in
    the pass's output block and must not count again."""
    from bundleadjustmentmatlab_amd._lib import VlgbaStats
    ptr = np.array([0, 2, 6, 11], dtype=np.int64)
    script = np.array([
        [[8, 2, 4, 0], [16, 8, 1, 0], [10, 5, 1, 0]],
        [[2, 3, 1, 0], [8, 4, 1, 1], [5, 2.5, 1, 0]],
        [[2, 2.5, 1, 1], [4, 3.999, 1, 0], [2.5, 1.25, 1, 0]],
        [[9, 1, 1, 1], [9, 1, 1, 1], [1.25, 0.5, 1, 1]],
    ], dtype=np.float64)
    opt, cap = _options(max_iter=5, max_iter2=2)
    x, err, nerr = np.full(3, -1.0), np.zeros((3, cap)), np.zeros(3, dtype=np.int32)
    st = VlgbaStats()
    rc = bh.bh_scripted(3, ptr.ctypes.data_as(_lp), ctypes.addressof(opt), len(script), _P(script),
                        _P(x), _P(err), cap, nerr.ctypes.data_as(_ip), ctypes.addressof(st))
    assert rc == 0
    assert (st.iterations, st.accepted, st.pinv_passes) == (3 + 3 + 4, 1 + 3 + 4, 3)
    assert nerr.tolist() == [2, 4, 5]
    assert np.array_equal(err[0, :2], [8 / 2, 2 / 2])
    assert np.array_equal(err[1, :4], [16 / 4, 8 / 4, 4 / 4, 3.999 / 4])
    assert np.array_equal(err[2, :5], [10 / 5, 5 / 5, 2.5 / 5, 1.25 / 5, 0.5 / 5])
    assert x.tolist() == [0.0, 1.0, 1.0]      # x_new where the last pass was accepted
    assert st.lambda_ == pytest.approx(1e-3 / 3 * 2 * 4, rel=1e-15)
