"""The host plan of the selected inverse on the cyclic-reduction factors
(vlgba_debug_selinv_plan, csrc/ba_chol_plan.cpp; VLGBA_COV_SELECTED): for tile
counts 1 .. 40 and 200 the returned elimination records and Sigma_qp sources
drive a numpy model of the descent

    Mp = Li^T Lp_e^T,  Mq = Li^T Lq_e^T
    Sigma_ep = -(Mp Sigma_pp + Mq Sigma_qp)
    Sigma_eq = -(Mp Sigma_qp^T + Mq Sigma_qq)
    Sigma_ee = Li^T Li - Sigma_ep Mp^T - Sigma_eq Mq^T

on a random SPD block-tridiagonal matrix with 4-row tiles; every diagonal and
sub-diagonal tile must match numpy.linalg.inv to 1e-12 of the tile's largest
entry.  The elimination order and every Sigma_qp lookup are taken from the
returned lists, never re-derived here.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4
COUNTS = list(range(1, 41)) + [200]


def selinv_plan(nt):
    from bundleadjustmentmatlab_amd import _lib
    L = _lib.lib()
    elim = np.zeros(3 * nt, dtype=np.int32)
    eptr = np.zeros(34, dtype=np.int32)
    src = np.zeros(2 * nt, dtype=np.int32)
    nl = L.vlgba_debug_selinv_plan(nt, elim.ctypes.data_as(_lib.c_ip),
                                   eptr.ctypes.data_as(_lib.c_ip), src.ctypes.data_as(_lib.c_ip))
    assert nl >= 1, nl
    return elim.reshape(nt, 3), eptr[: nl + 1], src.reshape(nt, 2)


def spd_tridiag(nt, rng):
    """Block-tridiagonal SPD, diagonally dominant (condition number of a few
    units: numpy.linalg.inv itself is then good to a few ulps, so the 1e-12 bar
    tests the plan and not the conditioning)."""
    n = T * nt
    A = np.zeros((n, n))
    for t in range(nt):
        G = 0.25 * rng.standard_normal((T, T))
        A[T * t:T * t + T, T * t:T * t + T] = 8.0 * np.eye(T) + G + G.T
        if t > 0:
            C = 0.4 * rng.standard_normal((T, T))
            A[T * t:T * t + T, T * t - T:T * t] = C
            A[T * t - T:T * t, T * t:T * t + T] = C.T
    return A


def tile(A, i, j):
    return A[T * i:T * i + T, T * j:T * j + T]


def factor(A, elim, eptr):
    """The cyclic reduction in the records' order: per record Li, Lp, Lq."""
    nt = len(elim)
    D = {t: tile(A, t, t).copy() for t in range(nt)}
    C = {}                                   # C[(hi, lo)] coupling of active neighbours
    for t in range(1, nt):
        C[(t, t - 1)] = tile(A, t, t - 1).copy()
    Li, Lp, Lq = {}, {}, {}
    for lev in range(len(eptr) - 1):
        for i in range(eptr[lev], eptr[lev + 1]):
            e, p, q = (int(v) for v in elim[i])
            Le = np.linalg.cholesky(D[e])
            Li[i] = np.linalg.inv(Le)
            if p >= 0:
                Lp[i] = C[(e, p)].T @ Li[i].T        # C(p, e) L_e^-T
                D[p] = D[p] - Lp[i] @ Lp[i].T
            if q >= 0:
                Lq[i] = C[(q, e)] @ Li[i].T          # C(q, e) L_e^-T
                D[q] = D[q] - Lq[i] @ Lq[i].T
            if p >= 0 and q >= 0:
                C[(q, p)] = -Lq[i] @ Lp[i].T
    return Li, Lp, Lq


def descent(elim, eptr, src, Li, Lp, Lq):
    nt = len(elim)
    See, Xp, Xq = {}, {}, {}
    for lev in range(len(eptr) - 2, -1, -1):
        for i in range(eptr[lev], eptr[lev + 1]):
            e, p, q = (int(v) for v in elim[i])
            W = Li[i].T @ Li[i]
            Mp = Li[i].T @ Lp[i].T if p >= 0 else None
            Mq = Li[i].T @ Lq[i].T if q >= 0 else None
            Sqp = None
            if p >= 0 and q >= 0:
                s, tr = int(src[i, 0]), int(src[i, 1])
                assert s >= 0
                Sqp = Xq[s].T if tr else Xp[s]       # the lookup rule, from the lists
            else:
                assert src[i, 0] == -1
            z = np.zeros((T, T))
            if p >= 0:
                Xp[i] = -(Mp @ See[p] + (Mq @ Sqp if q >= 0 else z))
            if q >= 0:
                Xq[i] = -((Mp @ Sqp.T if p >= 0 else z) + Mq @ See[q])
            S = W.copy()
            if p >= 0:
                S -= Xp[i] @ Mp.T
            if q >= 0:
                S -= Xq[i] @ Mq.T
            See[e] = S
    assert len(See) == nt
    return See, Xp, Xq


@pytest.mark.parametrize("nt", COUNTS)
def test_recurrence_matches_inverse(nt):
    elim, eptr, src = selinv_plan(nt)
    assert eptr[0] == 0 and eptr[-1] == nt
    assert sorted(elim[:, 0].tolist()) == list(range(nt))
    rng = np.random.default_rng(1000 + nt)
    A = spd_tridiag(nt, rng)
    want = np.linalg.inv(A)
    Li, Lp, Lq = factor(A, elim, eptr)
    See, Xp, Xq = descent(elim, eptr, src, Li, Lp, Lq)
    for t in range(nt):
        ref = tile(want, t, t)
        assert np.abs(See[t] - ref).max() <= 1e-12 * np.abs(ref).max(), t
    # sub-diagonal tiles: level 0's records
    seen = set()
    for i in range(eptr[0], eptr[1]):
        e, p, q = (int(v) for v in elim[i])
        if p >= 0:
            assert p == e - 1
            ref = tile(want, e, p)
            assert np.abs(Xp[i] - ref).max() <= 1e-12 * np.abs(ref).max(), (e, p)
            seen.add((e, p))
        if q >= 0:
            assert q == e + 1
            ref = tile(want, e, q)
            assert np.abs(Xq[i] - ref).max() <= 1e-12 * np.abs(ref).max(), (e, q)
            seen.add((q, e))
    # level 0 covers every adjacent pair (t + 1, t) exactly once
    assert sorted(seen) == [(t + 1, t) for t in range(nt - 1)]
    npairs = sum(int(elim[i, 1] >= 0) + int(elim[i, 2] >= 0) for i in range(eptr[0], eptr[1]))
    assert npairs == nt - 1


@pytest.mark.parametrize("nt", COUNTS)
def test_sources_are_neighbour_records(nt):
    """The source record is p's or q's, above e's level, with the other tile as
    its neighbour on the side the flag says."""
    elim, eptr, src = selinv_plan(nt)
    lev = np.zeros(nt, dtype=int)
    for l in range(len(eptr) - 1):
        lev[eptr[l]:eptr[l + 1]] = l
    for i in range(nt):
        e, p, q = (int(v) for v in elim[i])
        s, tr = int(src[i, 0]), int(src[i, 1])
        if p < 0 or q < 0:
            assert (s, tr) == (-1, 0)
            continue
        assert p < e < q and lev[s] > lev[i]
        if tr:
            assert elim[s, 0] == p and elim[s, 2] == q
        else:
            assert elim[s, 0] == q and elim[s, 1] == p


def test_binding_declares_selected_method():
    """The header and the library agree on the new entry points (ABI 6: entry
    points only), and each refuses a NULL context."""
    from bundleadjustmentmatlab_amd import _lib
    with open(os.path.join(ROOT, "include", "vlgba.h")) as f:
        hdr = f.read()
    assert "#define VLGBA_COV_DENSE 0" in hdr and "#define VLGBA_COV_SELECTED 1" in hdr
    assert "int vlgba_set_covariance_method(vlgba_ctx *ctx, int kind);" in hdr
    assert "int vlgba_get_covariance_method(vlgba_ctx *ctx, int *kind);" in hdr
    assert "int vlgba_get_covariance_blocks(vlgba_ctx *ctx, int *blk_jk, double *blocks);" in hdr
    assert "int vlgba_debug_selinv_plan(int ntiles, int *elim, int *eptr, int *src);" in hdr
    assert _lib.ABI_VERSION == 6 and "#define VLGBA_ABI_VERSION 6" in hdr
    assert _lib.COV_METHODS == {"dense": 0, "selected": 1}
    L = _lib.lib()
    assert L.vlgba_set_covariance_method.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.vlgba_get_covariance_method.argtypes == [ctypes.c_void_p, _lib.c_ip]
    assert L.vlgba_get_covariance_blocks.argtypes == [ctypes.c_void_p, _lib.c_ip, _lib.c_dp]
    assert L.vlgba_debug_selinv_plan.argtypes == [ctypes.c_int] + [_lib.c_ip] * 3
    kind = ctypes.c_int(7)
    assert L.vlgba_set_covariance_method(None, 0) == -1001
    assert L.vlgba_set_covariance_method(None, 1) == -1001
    assert L.vlgba_get_covariance_method(None, ctypes.byref(kind)) == -1001
    assert L.vlgba_get_covariance_blocks(None, None, None) == -1001
    assert kind.value == 7
    assert L.vlgba_debug_selinv_plan(0, None, None, None) == -1


def test_python_api_has_method_switch():
    import inspect
    from bundleadjustmentmatlab_amd import bundle, projective
    sig = inspect.signature(bundle.BundleAdjuster.covariance)
    assert sig.parameters["method"].default is None and sig.parameters["blocks"].default is False
    assert hasattr(bundle.BundleAdjuster, "set_covariance_method")
    for fn in (bundle.bundle_euclid_obs, bundle.bundle_euclid, bundle.bundle_euclid_nomex,
               projective.bundle_projective_obs, projective.bundle_projective):
        assert inspect.signature(fn).parameters["covariance_method"].default is None


def test_planner_under_sanitizer(tmp_path):
    """tests/native/selinv_plan_host.cpp + the host planner as one stand-alone
    program under AddressSanitizer + UndefinedBehaviorSanitizer: the same tile
    counts into exactly-sized arrays."""
    import plan_cases as pc
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    b = subprocess.run([pc.CXX, *flags, str(probe), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    if b.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("an empty AddressSanitizer program does not build or run here")
    exe = tmp_path / "selinv_plan_host"
    b = pc.build_harness(exe, flags, [os.path.join(ROOT, "tests", "native", "selinv_plan_host.cpp"),
                                      pc.CHOL_SOURCES[2]])
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for bad in ("AddressSanitizer", "runtime error"):
        assert bad not in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("selinv ")]
    assert [int(t[1]) for t in lines] == COUNTS
    for t in lines:
        assert int(t[2]) == len(selinv_plan(int(t[1]))[1]) - 1
