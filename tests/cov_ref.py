"""Extended-precision reference of the posterior covariances
(vlgba_covariance) -- TEST INFRASTRUCTURE ONLY, in the style of schur_ref.py
(whose long double Schur complement it starts from):

    inverse_ld   Sigma_a = S0^-1 of the undamped reduced camera system, by a
                 long double Cholesky factorisation (fixed rows: unit diagonal
                 for the factorisation, zero rows and columns in the result)
    point_cov    Sigma_b_i = V+_i + V+_i T_i V+_i,
                 T_i = sum_{j,k in cams(i)} W_ij^T Sigma_a[j,k] W_ik,
                 in long double from the fp64 W, V+ and Sigma_a it is GIVEN
                 (the code under test's own upstream outputs), with a per-entry
                 rounding bound for an fp64 evaluation

V+ is not recomputed: it is the fp64 closed form the device uses
(schur_ref.vinv_of(V, 0)), passed in by the caller.  Both the kernel and this
reference compute the lower entries of Sigma_b_i from the stored V+ and mirror
them, so the result is symmetric whatever the last bits of V+ are.
"""
import numpy as np

import schur_ref as sr

LD = sr.LD
U53 = sr.U53


def apply_pivot(lin, cam, pivot):
    """bundle_euclid.m:150-154 on a linearisation dict (U (na, na, m), eA
    (na, m), W (na, 3, N)): the pivot cameras' U, eA and W are zero."""
    pivot = np.asarray(pivot, dtype=bool)
    out = dict(lin)
    out["U"] = np.array(lin["U"], order="F")
    out["eA"] = np.array(lin["eA"], order="F")
    out["W"] = np.array(lin["W"], order="F")
    out["U"][:, :, pivot] = 0.0
    out["eA"][:, pivot] = 0.0
    out["W"][:, :, pivot[np.asarray(cam)]] = 0.0
    return out


def dense_lower(ref):
    """The dense lower triangle (long double, ld x ld) of a schur_ref.schur
    result."""
    na, m = ref["na"], ref["m"]
    S = np.zeros((na * m, na * m), dtype=LD)
    for (j, k), B in zip(ref["jk"], ref["S"]):
        S[na * j:na * j + na, na * k:na * k + na] = np.tril(B) if j == k else B
    return S


def schur_fp64(m, na, pt, cam, W, Vinv, U):
    """S0 = U - sum_i W_i V+_i W_i^T formed in plain fp64 (numpy's order): the
    full symmetric (na m, na m) matrix an fp64 implementation starts from.  It
    carries the Schur complement's own fp64 rounding, which the rounded long
    double S0 does not; the fp64 routes that set the tests' bars invert this
    one."""
    pt = np.asarray(pt, dtype=np.int64)
    cam = np.asarray(cam, dtype=np.int64)
    N = len(pt)
    Wn = np.asarray(W, dtype=np.float64).reshape(na, 3, N, order="F").transpose(2, 0, 1)
    Vi = np.asarray(Vinv, dtype=np.float64).transpose(2, 0, 1)[pt]
    Y = np.einsum("orq,oqc->orc", Wn, Vi)
    S = np.zeros((na * m, na * m))
    for j in range(m):
        S[na * j:na * j + na, na * j:na * j + na] = np.tril(np.asarray(U)[:, :, j])
    oa, ob = sr._pairs(pt)
    if len(oa):
        key = cam[oa] * m + cam[ob]
        order = np.argsort(key, kind="stable")
        oa, ob, key = oa[order], ob[order], key[order]
        st = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        sums = np.add.reduceat(np.einsum("prq,pcq->prc", Y[oa], Wn[ob]), st, axis=0)
        for (j, k), B in zip(np.stack([key[st] // m, key[st] % m], 1), sums):
            S[na * j:na * j + na, na * k:na * k + na] -= np.tril(B) if j == k else B
    return sr.symmetrise(S)


def inverse_fp64(S, fixed_rows):
    """numpy.linalg.inv of the free rows and columns of a symmetric S, zeros
    elsewhere, the lower triangle mirrored."""
    free = np.flatnonzero(~np.asarray(fixed_rows, dtype=bool))
    inv = np.zeros_like(S)
    if len(free):
        inv[np.ix_(free, free)] = np.linalg.inv(S[np.ix_(free, free)])
    return np.tril(inv) + np.tril(inv, -1).T


def fixed_rows_of(S_lower):
    """The exactly-zero rows of S0: those with a zero diagonal (App. A Q2, Q8:
    the rule of k_fix_diag)."""
    return np.diag(np.asarray(S_lower)) == 0


def inverse_ld(S_lower, fixed_rows):
    """S^-1 (full, symmetric, long double) of the symmetric positive definite
    matrix whose lower triangle is S_lower, by Cholesky: L column by column,
    X = L^-1 row by row (each step one vectorised product), S^-1 = X^T X.  Rows
    in ``fixed_rows`` (bool mask) are taken out (unit diagonal) and are zero
    rows and columns of the result.  For ld up to a few hundred."""
    A = np.array(S_lower, dtype=LD)
    ld = A.shape[0]
    fixed = np.asarray(fixed_rows, dtype=bool)
    A = np.tril(A)
    A[fixed, :] = 0
    A[:, fixed] = 0
    A[fixed, fixed] = 1
    L = np.zeros((ld, ld), dtype=LD)
    for j in range(ld):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"non-positive pivot in column {j}")
        L[j:, j] = col / np.sqrt(col[0])
    X = np.zeros((ld, ld), dtype=LD)
    eye = np.eye(ld, dtype=LD)
    for i in range(ld):
        X[i, :i + 1] = (eye[i, :i + 1] - L[i, :i] @ X[:i, :i + 1]) / L[i, i]
    inv = X.T @ X
    inv = np.tril(inv) + np.tril(inv, -1).T
    inv[fixed, :] = 0
    inv[:, fixed] = 0
    return inv


def chain_length(na, track):
    """k of point_cov's bound: the longest chain of fp64 roundings behind an
    entry of Sigma_b_i in k_point_cov's summation order,

        k = 2 na + ceil(P / 8) + 13,    P = track (track + 1) / 2 pairs j >= k:

    na for Sigma_a[j,k] W_ik (na terms, product and sum counted apart although
    the kernel fuses them: the bound holds with or without fma), na for W_ij^T
    times that, 1 for M + M^T, ceil(P / LPP) for a lane's running sum over its
    pairs and log2(LPP) for the butterfly over the LPP lanes of a point
    (LPP = 8, 64 or 256 by track length; 8 gives the largest total for every
    track the wider forms take), 3 + 3 for the two 3-term products with V+
    and 1 for the final addition to V+, with one to spare."""
    track = np.asarray(track, dtype=np.int64)
    return 2 * na + -(-(track * (track + 1) // 2) // 8) + 13


def _sym_lower(M):
    """(.., 3, 3): the lower entries mirrored."""
    low = np.tril(np.ones((3, 3), dtype=bool))
    return np.where(low, M, np.swapaxes(M, -1, -2))


def point_cov(na, pt, cam, W, Vinv, cov_a_full):
    """(Sigma_b (3, 3, n) long double, bound (3, 3, n)) from the fp64 W
    (na, 3, N; observations point-major, cameras ascending within a point),
    Vinv (3, 3, n) and the full symmetric cov_a_full (ld, ld).

    bound = gamma_k (|V+| + |V+| (sum_jk |W_ij|^T |Sigma_a[j,k]| |W_ik|) |V+|),
    gamma_k = k u / (1 - k u), k = chain_length(na, track of the point): the
    sum of the absolute values of every product that enters the entry, times
    the rounding of the longest chain of operations the kernel's order allows.
    An entry whose bound is zero must be exact (unseen points, fix_structure).
    """
    pt = np.asarray(pt, dtype=np.int64)
    cam = np.asarray(cam, dtype=np.int64)
    N = len(pt)
    Vinv = np.asarray(Vinv, dtype=np.float64)
    n = Vinv.shape[2]
    Sa = np.asarray(cov_a_full, dtype=np.float64)
    assert np.array_equal(Sa, Sa.T), "cov_a_full must be exactly symmetric"
    Wl = np.asarray(W, dtype=np.float64).reshape(na, 3, N, order="F").transpose(2, 0, 1)
    T = np.zeros((n, 3, 3), dtype=LD)
    Ta = np.zeros((n, 3, 3), dtype=LD)
    track = np.bincount(pt, minlength=n)
    if N:
        assert np.all((np.diff(pt) > 0) | ((np.diff(pt) == 0) & (np.diff(cam) > 0)))
        first = np.flatnonzero(np.r_[True, pt[1:] != pt[:-1]])
        L = np.diff(np.r_[first, N])
        ar = np.arange(na)
        for t in np.unique(L):
            starts = first[L == t]
            step = max(1, int(2_000_000 // (t * t * na * na)))
            for q0 in range(0, len(starts), step):
                s = starts[q0:q0 + step]
                o = s[:, None] + np.arange(t)[None, :]                     # (p, t)
                w = Wl[o].astype(LD)                                       # (p, t, na, 3)
                rows = (cam[o] * na)[:, :, None] + ar[None, None, :]       # (p, t, na)
                blk = Sa[rows[:, :, None, :, None], rows[:, None, :, None, :]].astype(LD)
                G = np.einsum("pjkab,pkbc->pjac", blk, w)
                Ga = np.einsum("pjkab,pkbc->pjac", np.abs(blk), np.abs(w))
                T[pt[s]] = np.einsum("pjar,pjac->prc", w, G)
                Ta[pt[s]] = np.einsum("pjar,pjac->prc", np.abs(w), Ga)
    Vi = Vinv.transpose(2, 0, 1).astype(LD)                                # (n, r, c)
    cov = Vi + np.einsum("nrs,nst,ntc->nrc", Vi, T, Vi)
    mag = np.abs(Vi) + np.einsum("nrs,nst,ntc->nrc", np.abs(Vi), Ta, np.abs(Vi))
    k = chain_length(na, track).astype(LD) * LD(U53)
    bound = (k / (1 - k))[:, None, None] * mag
    return _sym_lower(cov).transpose(1, 2, 0), _sym_lower(bound).transpose(1, 2, 0)


def point_cov_fp64(na, pt, cam, W, Vi, cov_a):
    """The point formula in plain fp64 over all ordered pairs, in numpy's order
    (an fp64 route of its own: the two-route floors of the tests)."""
    n = Vi.shape[2]
    out = np.zeros((3, 3, n))
    ptr = np.r_[0, np.cumsum(np.bincount(pt, minlength=n))]
    for i in range(n):
        T = np.zeros((3, 3))
        o = range(ptr[i], ptr[i + 1])
        for oj in o:
            for ok in o:
                j, k = cam[oj], cam[ok]
                T += W[:, :, oj].T @ cov_a[na * j:na * j + na, na * k:na * k + na] @ W[:, :, ok]
        out[:, :, i] = Vi[:, :, i] + Vi[:, :, i] @ T @ Vi[:, :, i]
    return out


def point_ratio(cov_b, ref, bound):
    return sr._ratio(np.asarray(cov_b, dtype=np.float64).astype(LD) - ref, bound)


def block_figure(got, ref, size):
    """The largest per-block max|got - ref| / max|ref block| over the
    size x size blocks of a square matrix, or over a (size, size, count) stack
    (blocks whose reference is zero must be zero: inf otherwise)."""
    got = np.asarray(got, dtype=LD)
    ref = np.asarray(ref, dtype=LD)
    if got.ndim == 2:
        nb = got.shape[0] // size
        got = got.reshape(nb, size, nb, size).transpose(0, 2, 1, 3).reshape(-1, size, size)
        ref = ref.reshape(nb, size, nb, size).transpose(0, 2, 1, 3).reshape(-1, size, size)
    else:
        got, ref = got.transpose(2, 0, 1), ref.transpose(2, 0, 1)
    d = np.abs(got - ref).max(axis=(1, 2))
    r = np.abs(ref).max(axis=(1, 2))
    fig = np.where(r > 0, d / np.where(r > 0, r, 1), np.where(d > 0, np.inf, 0))
    return float(fig.max()) if fig.size else 0.0


def diag_blocks(full, na):
    """(na, na, m) diagonal blocks of a (na m, na m) matrix."""
    full = np.asarray(full)
    m = full.shape[0] // na
    return np.stack([full[na * j:na * j + na, na * j:na * j + na] for j in range(m)], axis=2)


def normal_inverse(na, m, n, pt, cam, U, V, W, fixed_rows, seen):
    """The independent route: numpy.linalg.inv of the full normal matrix
    [[U, W], [W^T, V]] (fp64) with the fixed camera rows and the unseen points'
    rows taken out -> (Sigma_a (ld, ld), Sigma_b (3, 3, n)) with zeros there."""
    ld = na * m
    H = np.zeros((ld + 3 * n, ld + 3 * n))
    Wn = np.asarray(W, dtype=np.float64).reshape(na, 3, -1, order="F")
    for j in range(m):
        H[na * j:na * j + na, na * j:na * j + na] = U[:, :, j]
    for i in range(n):
        H[ld + 3 * i:ld + 3 * i + 3, ld + 3 * i:ld + 3 * i + 3] = V[:, :, i]
    for o, (i, j) in enumerate(zip(pt, cam)):
        H[na * j:na * j + na, ld + 3 * i:ld + 3 * i + 3] = Wn[:, :, o]
        H[ld + 3 * i:ld + 3 * i + 3, na * j:na * j + na] = Wn[:, :, o].T
    keep = np.r_[~np.asarray(fixed_rows, dtype=bool), np.repeat(np.asarray(seen, dtype=bool), 3)]
    idx = np.flatnonzero(keep)
    inv = np.zeros_like(H)
    inv[np.ix_(idx, idx)] = np.linalg.inv(H[np.ix_(idx, idx)])
    cov_b = np.stack([inv[ld + 3 * i:ld + 3 * i + 3, ld + 3 * i:ld + 3 * i + 3] for i in range(n)],
                     axis=2)
    return inv[:ld, :ld], cov_b, H
