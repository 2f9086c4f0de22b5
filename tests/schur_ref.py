"""Extended-precision reference of the three stages behind one LM pass --
TEST INFRASTRUCTURE ONLY (a plain helper module like scene_ref.py).

Every function takes the UPSTREAM outputs of the code under test (the
linearisation's U / V / W / eA / eB, the solver's da) and restates one stage
in numpy long double (80-bit: 64-bit significand), together with a rigorous
per-entry rounding bound for an fp64 evaluation of the same stage, so a stage
is judged alone and entry by entry:

    schur       S_jk = U*_j [j == k] - sum_i Y_ij W_ik^T,  e_j = eA_j - sum_i Y_ij eB_i
    residual    componentwise backward error of S da = e_ (residual_blocks: the
                same from the blocks, without the dense S)
    back_subst  db_i = V*^-1_i (eB_i - sum_j W_ij^T da_j[:ndb])

The bounds count roundings and multiply by the sum of absolute values of the
terms (the standard running-error form): an entry that is the sum of t
products, each of operands carrying a few roundings of their own, is within
(t + c) u sum|terms| of the exact value in ANY summation order, with or without
fused multiply-adds, u = 2^-53.  They need no measurement and scale with each
entry's own terms: a block with three co-visible points is held to three
points' rounding, not to the largest entry of S.

V*^-1 is NOT recomputed in long double: it is the fp64 closed form the device
uses (vlg_pinv3 == oracle.pinv3_formula, the same expression compiled without
contraction on both sides), passed in by the caller, so its own conditioning
does not enter the bounds.  k_damp_point, k_schur_group and k_point_vinv (the
V*^-1 of k_schur_mfma and of the long tracks) all call vlg_pinv3 on
(1 + lambda) * diag(V) -- no fast-path kernel has a V*^-1 of its own.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "schur_ref needs an 80-bit (or wider) long double"
U53 = 2.0 ** -53     # unit roundoff of fp64


def damp(M, lam):
    """(1 + lam) * diag in fp64, as the device and bundle_euclid.m:168-176 do;
    M is (k, k, count)."""
    M = np.array(M, dtype=np.float64, order="F")
    for q in range(M.shape[0]):
        M[q, q] = (1 + lam) * M[q, q]
    return M


def _pairs(pt):
    """(oa, ob) of every two observations of one point with oa >= ob (itself
    included); pt sorted ascending."""
    pt = np.asarray(pt)
    N = len(pt)
    if N == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z
    assert np.all(np.diff(pt) >= 0), "observations must be point-major"
    first = np.flatnonzero(np.r_[True, pt[1:] != pt[:-1]])
    L = np.diff(np.r_[first, N])
    oa, ob = [], []
    for l in np.unique(L):
        s = first[L == l]
        r, c = np.tril_indices(int(l))
        oa.append((s[:, None] + r[None, :]).reshape(-1))
        ob.append((s[:, None] + c[None, :]).reshape(-1))
    return np.concatenate(oa), np.concatenate(ob)


def _obs_y(na, pt, W, Vinv):
    """Per observation, in long double: W_o (N, na, 3), Y_o = W_o V*^-1 and
    |W_o| |V*^-1|."""
    N = len(pt)
    Wl = np.asarray(W, dtype=np.float64).reshape(na, 3, N, order="F").transpose(2, 0, 1).astype(LD)
    Vi = np.asarray(Vinv, dtype=np.float64).transpose(2, 0, 1).astype(LD)[np.asarray(pt)]
    Y = np.einsum("orq,oqc->orc", Wl, Vi)
    Ya = np.einsum("orq,oqc->orc", np.abs(Wl), np.abs(Vi))
    return Wl, Y, Ya


def vinv_of(V, lam):
    """V*^-1: the oracle's fp64 closed form (orc_pinv3_formula, the same
    expression as the device's vlg_pinv3) on the damped V."""
    import bundle_euclid_ref as oracle
    return oracle.pinv3_formula(damp(V, lam))


def schur(m, n, na, pt, cam, W, V, eB, U, eA, lam, Vinv=None):
    """The reduced camera system of mex_bundle_2_Se_.c on an observation list
    (pt, cam sorted point-major, cameras ascending within a point), from the
    UNDAMPED fp64 stage-1 outputs U (na, na, m), V (3, 3, n), W (na, 3, N),
    eA (na, m), eB (3, n); Vinv (3, 3, n) defaults to vinv_of(V, lam).

    Returns a dict: jk (nb, 2) the co-visible blocks j >= k (every diagonal
    block included), S (nb, na, na) [b, r, c] and bound (same shape), npts
    (nb,), e (na * m,) and ebound.

    bound_jk = (3 npts_jk + 8) u A_jk, A_jk = sum_i |W_ij| |V*^-1_i| |W_ik|^T
    (+ |U*_j|): 3 npts is the longest chain of additions an entry can see
    (three products per point), 8 covers the roundings of Y (3), of each
    product (1), of the damping (1) and of the final subtraction (1) with
    room for the second-order terms.  ebound_j likewise with 3 nobs_j + 8."""
    pt = np.asarray(pt, dtype=np.int64)
    cam = np.asarray(cam, dtype=np.int64)
    N = len(pt)
    if N > 1:
        assert np.all((np.diff(pt) > 0) | ((np.diff(pt) == 0) & (np.diff(cam) > 0)))
    Us = damp(U, lam)
    if Vinv is None:
        Vinv = vinv_of(V, lam)
    Wl, Y, Ya = _obs_y(na, pt, W, Vinv)
    Wa = np.abs(Wl)
    oa, ob = _pairs(pt)
    key = cam[oa] * m + cam[ob]
    diag = np.arange(m, dtype=np.int64) * (m + 1)
    keys = np.unique(np.r_[key, diag])
    nb = len(keys)
    S = np.zeros((nb, na, na), dtype=LD)
    A = np.zeros((nb, na, na), dtype=LD)
    npts = np.zeros(nb, dtype=np.int64)
    order = np.argsort(key, kind="stable")
    oa, ob, bidx = oa[order], ob[order], np.searchsorted(keys, key[order])
    step = 1 << 15
    for p0 in range(0, len(oa), step):
        a, b, bi = oa[p0:p0 + step], ob[p0:p0 + step], bidx[p0:p0 + step]
        st = np.flatnonzero(np.r_[True, bi[1:] != bi[:-1]])
        ub = bi[st]
        S[ub] -= np.add.reduceat(np.einsum("prq,pcq->prc", Y[a], Wl[b]), st, axis=0)
        A[ub] += np.add.reduceat(np.einsum("prq,pcq->prc", Ya[a], Wa[b]), st, axis=0)
        npts[ub] += np.diff(np.r_[st, len(bi)])
    dblk = np.searchsorted(keys, diag)
    Ul = np.asarray(Us).transpose(2, 0, 1).astype(LD)
    S[dblk] += Ul
    A[dblk] += np.abs(Ul)
    bound = ((3 * npts + 8) * U53)[:, None, None] * A
    # e_
    eBl = np.asarray(eB, dtype=np.float64).T.astype(LD)[pt]            # (N, 3)
    e = np.asarray(eA, dtype=np.float64).T.astype(LD).copy()           # (m, na)
    Ae = np.abs(e)
    te = np.einsum("orc,oc->or", Y, eBl)
    ta = np.einsum("orc,oc->or", Ya, np.abs(eBl))
    co = np.argsort(cam, kind="stable")
    nobs = np.bincount(cam, minlength=m)
    if N:
        st = np.flatnonzero(np.r_[True, cam[co][1:] != cam[co][:-1]])
        uc = cam[co][st]
        e[uc] -= np.add.reduceat(te[co], st, axis=0)
        Ae[uc] += np.add.reduceat(ta[co], st, axis=0)
    ebound = ((3 * nobs + 8) * U53)[:, None] * Ae
    jk = np.stack([keys // m, keys % m], 1)
    return dict(jk=jk, S=S, bound=bound, npts=npts, e=e.reshape(-1), ebound=ebound.reshape(-1),
                na=na, m=m)


def _ratio(diff, bound):
    """max |diff| / bound; an entry with a zero bound must be exact."""
    diff = np.abs(np.asarray(diff, dtype=LD))
    bound = np.asarray(bound, dtype=LD)
    if diff.size == 0:
        return 0.0
    r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0))
    return float(r.max())


def blocks_of(S, jk, na):
    """The (nb, na, na) blocks [b, r, c] of a dense S at the block indices jk."""
    S = np.asarray(S)
    return np.stack([S[na * j:na * j + na, na * k:na * k + na] for j, k in jk]) if len(jk) \
        else np.zeros((0, na, na))


def schur_ratio(ref, jk, blocks, e_):
    """(max |S - ref| / bound, max |e_ - ref| / ebound) of a computed reduced
    system given as blocks (jk (nb, 2), blocks (nb, na, na) [b, r, c], j >= k;
    only the lower triangle of a diagonal block is read).  A block the
    reference does not have must be exactly zero, and a non-zero block of the
    reference that is missing counts as computed zero: either gives inf when
    violated."""
    na, m = ref["na"], ref["m"]
    jk = np.asarray(jk, dtype=np.int64).reshape(-1, 2)
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, na, na)
    assert np.all(jk[:, 0] >= jk[:, 1]) and np.all(jk >= 0) and np.all(jk < m), "block index"
    key = jk[:, 0] * m + jk[:, 1]
    assert len(np.unique(key)) == len(key), "a block returned twice"
    rkey = ref["jk"][:, 0] * m + ref["jk"][:, 1]
    pos = np.searchsorted(rkey, key)
    pos = np.minimum(pos, len(rkey) - 1)
    known = rkey[pos] == key
    low = np.tril(np.ones((na, na), dtype=bool))
    worst = 0.0
    if np.any(blocks[~known] != 0.0):
        worst = np.inf
    seen = np.zeros(len(rkey), dtype=bool)
    seen[pos[known]] = True
    mask = np.where((jk[known, 0] == jk[known, 1])[:, None, None], low[None], True)
    d = (blocks[known].astype(LD) - ref["S"][pos[known]]) * mask
    worst = max(worst, _ratio(d, ref["bound"][pos[known]]))
    # blocks the computation did not return: as if returned zero
    miss = ~seen
    mmask = np.where((ref["jk"][miss, 0] == ref["jk"][miss, 1])[:, None, None], low[None], True)
    worst = max(worst, _ratio(ref["S"][miss] * mmask, ref["bound"][miss]))
    we = _ratio(np.asarray(e_, dtype=np.float64).reshape(-1).astype(LD) - ref["e"], ref["ebound"])
    return worst, we


def symmetrise(S_lower):
    S = np.asarray(S_lower, dtype=np.float64)
    return np.tril(S) + np.tril(S, -1).T


def residual(S_lower_dense, e_, da, rows=None):
    """Componentwise backward error of da as the solution of S da = e_
    (Oettli-Prager): max_r |S da - e_|_r / (|S| |da| + |e_|)_r in long double
    on the symmetrised S, over ``rows`` (a bool mask; default all).  A row
    whose numerator and denominator are both zero counts as zero."""
    S = symmetrise(S_lower_dense).astype(LD)
    e = np.asarray(e_, dtype=np.float64).reshape(-1).astype(LD)
    x = np.asarray(da, dtype=np.float64).reshape(-1, order="F").astype(LD)
    num = np.abs(S @ x - e)
    den = np.abs(S) @ np.abs(x) + np.abs(e)
    if rows is not None:
        num, den = num[rows], den[rows]
    if num.size == 0:
        return 0.0
    r = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0))
    return float(r.max())


def residual_blocks(m, na, jk, blocks, e_, da, rows=None):
    """residual() without the dense S: the same Oettli-Prager quantity from the
    getter's blocks (jk (nb, 2) camera pairs j >= k, each once; blocks
    (nb, na, na) [b, r, c]; only the lower triangle of a diagonal block is
    read and mirrored, an off-diagonal block also acts transposed on rows k),
    numerator and denominator accumulated block by block in long double, the
    same 0 / 0 rule, ``rows`` a bool mask over the na * m rows.

    The sums are the dense product's terms in another order (a row's terms
    inside a block first, then the blocks in jk's order; the dense product
    adds a row's zeros too, exactly), so the two values agree to the rounding
    of the sums and not to the last bit: residual_slack() bounds the
    difference."""
    jk = np.asarray(jk, dtype=np.int64).reshape(-1, 2)
    B = np.asarray(blocks, dtype=np.float64).reshape(-1, na, na).astype(LD)
    assert len(B) == len(jk), "one block per index pair"
    assert np.all(jk[:, 0] >= jk[:, 1]) and np.all(jk >= 0) and np.all(jk < m), "block index"
    key = jk[:, 0] * m + jk[:, 1]
    assert len(np.unique(key)) == len(key), "a block returned twice"
    e = np.asarray(e_, dtype=np.float64).reshape(-1).astype(LD)
    x = np.asarray(da, dtype=np.float64).reshape(-1, order="F").astype(LD)
    assert e.size == na * m and x.size == na * m
    xc, xa = x.reshape(m, na), np.abs(x).reshape(m, na)
    sx = np.zeros((m, na), dtype=LD)       # S x
    ax = np.zeros((m, na), dtype=LD)       # |S| |x|
    dg = jk[:, 0] == jk[:, 1]
    D = np.tril(B[dg]) + np.tril(B[dg], -1).transpose(0, 2, 1)
    j = jk[dg, 0]
    np.add.at(sx, j, np.einsum("brc,bc->br", D, xc[j]))
    np.add.at(ax, j, np.einsum("brc,bc->br", np.abs(D), xa[j]))
    O, j, k = B[~dg], jk[~dg, 0], jk[~dg, 1]
    np.add.at(sx, j, np.einsum("brc,bc->br", O, xc[k]))
    np.add.at(ax, j, np.einsum("brc,bc->br", np.abs(O), xa[k]))
    np.add.at(sx, k, np.einsum("brc,br->bc", O, xc[j]))
    np.add.at(ax, k, np.einsum("brc,br->bc", np.abs(O), xa[j]))
    num = np.abs(sx.reshape(-1) - e)
    den = ax.reshape(-1) + np.abs(e)
    if rows is not None:
        num, den = num[rows], den[rows]
    if num.size == 0:
        return 0.0
    r = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0))
    return float(r.max())


def residual_slack(terms, eta=0.0):
    """How far residual() and residual_blocks() of the same system can lie
    apart, ``terms`` the most non-zero entries of a row of the symmetrised S.
    Each computed row sum of t terms is within gamma = t * eps of the exact one
    relative to sum |terms| <= den in any order (eps = 2^-64, the long double's
    unit roundoff), so the two numerators differ by at most 2 (t + 1) eps den
    (e_'s subtraction included), the two denominators by 2 t eps den, the
    quotients by (2 (t + 1) + 2 t eta) eps plus the division's rounding; the
    conversion of each result to fp64 adds 2^-53 eta.  Rounded up:
    3 (t + 2) eps + 2^-51 eta."""
    return 3.0 * (terms + 2) * 2.0 ** -64 + 2.0 ** -51 * eta


def back_subst(na, ndb, pt, cam, W, Vinv, eB, da):
    """db_i = V*^-1_i (eB_i - sum_j W_ij^T da_j[:ndb]) (mex_bundle_3_db_new.c:
    99-131 with ndb = 6 -- its six hard-coded terms, whatever num_a -- and
    bundle_euclid_nomex.m:268-277 with ndb = num_a) -> (db (3, n) long double,
    dbbound (3, n)).

    dbbound_i = (ndb L_i + 8) u |V*^-1_i| (|eB_i| + sum_j |W_ij|^T |da_j|),
    L_i the track length: ndb L_i bounds the chain of additions of the inner
    sums, 8 covers the products, the subtraction from eB and the 3-term
    product with V*^-1."""
    pt = np.asarray(pt, dtype=np.int64)
    cam = np.asarray(cam, dtype=np.int64)
    N = len(pt)
    n = np.asarray(eB).shape[1]
    Wl = np.asarray(W, dtype=np.float64).reshape(na, 3, N, order="F").transpose(2, 0, 1).astype(LD)
    d = np.asarray(da, dtype=np.float64).reshape(na, -1, order="F").T.astype(LD)[cam]   # (N, na)
    t = np.einsum("okc,ok->oc", Wl[:, :ndb], d[:, :ndb])
    ta = np.einsum("okc,ok->oc", np.abs(Wl[:, :ndb]), np.abs(d[:, :ndb]))
    rhs = np.asarray(eB, dtype=np.float64).T.astype(LD).copy()          # (n, 3)
    ra = np.abs(rhs)
    L = np.bincount(pt, minlength=n)
    if N:
        assert np.all(np.diff(pt) >= 0)
        st = np.flatnonzero(np.r_[True, pt[1:] != pt[:-1]])
        up = pt[st]
        rhs[up] -= np.add.reduceat(t, st, axis=0)
        ra[up] += np.add.reduceat(ta, st, axis=0)
    Vi = np.asarray(Vinv, dtype=np.float64).transpose(2, 0, 1).astype(LD)   # (n, r, c)
    db = np.einsum("nrc,nc->nr", Vi, rhs)
    bound = ((ndb * L + 8) * U53)[:, None] * np.einsum("nrc,nc->nr", np.abs(Vi), ra)
    return db.T, bound.T


def db_ratio(db, ref_db, bound):
    return _ratio(np.asarray(db, dtype=np.float64).astype(LD) - ref_db, bound)
