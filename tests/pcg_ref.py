"""Block-Jacobi PCG on the reduced camera system, restated in numpy --
TEST INFRASTRUCTURE ONLY (a plain helper module like schur_ref.py).

The system is given exactly as BundleAdjuster.reduced_system(dense=False)
returns it: jk (nb, 2) camera pairs j >= k, blocks (nb, na, na) indexed
[b, r, c] (only the lower triangle of a diagonal block is read and mirrored; an
off-diagonal block also acts transposed on the rows of k), e_ (na * m,).

    pcg          the algorithm of csrc/ba_pcg.hip in fp64, in numpy's own
                 summation order: the zero-row rule, M_j = the diagonal block of
                 camera j, the plain recurrences with rz = r' M^-1 r from da = 0,
                 stop after iteration k when sqrt(rz_k / rz_0) <= tol or k ==
                 max_iter; the failure conditions come back as status 4
    true_relres  sqrt(r' M^-1 r / e_' M^-1 e_) of a given da, r = e_ - S da
                 recomputed from the matrix in long double
    direct       the solution of the same system (zero-row rule applied) to long
                 double accuracy: LAPACK solves refined on long double residuals

Zero-row rule (k_fix_diag's, on blocks): a row whose diagonal entry in its
camera's diagonal block is exactly 0 -- or whose camera has no diagonal block --
gets a unit diagonal, zeros elsewhere in its row and column, and a zero
right-hand side; da is exactly 0 there.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "pcg_ref needs an 80-bit (or wider) long double"


class System:
    """The blocks split into what the iteration needs, in ``dtype``."""

    def __init__(self, jk, blocks, e_, dtype=np.float64):
        jk = np.asarray(jk, dtype=np.int64).reshape(-1, 2)
        B = np.asarray(blocks, dtype=np.float64)
        na = B.shape[-1]
        B = B.reshape(-1, na, na).astype(dtype)
        e = np.asarray(e_, dtype=np.float64).reshape(-1).astype(dtype)
        m = e.size // na
        assert e.size == na * m and len(B) == len(jk), "one block per index pair"
        assert np.all(jk[:, 0] >= jk[:, 1]) and np.all(jk >= 0) and np.all(jk < m), "block index"
        key = jk[:, 0] * m + jk[:, 1]
        assert len(np.unique(key)) == len(key), "a block given twice"
        self.m, self.na, self.dtype = m, na, dtype
        dg = jk[:, 0] == jk[:, 1]
        self.D = np.zeros((m, na, na), dtype=dtype)          # symmetric diagonal blocks
        self.D[jk[dg, 0]] = np.tril(B[dg]) + np.tril(B[dg], -1).transpose(0, 2, 1)
        self.O, self.oj, self.ok = B[~dg], jk[~dg, 0], jk[~dg, 1]
        self.fixed = np.einsum("jrr->jr", self.D) == 0        # (m, na)
        self.e = np.where(self.fixed, dtype(0), e.reshape(m, na))
        # M_j: the diagonal block with the rule applied
        M = self.D.copy()
        M[self.fixed[:, :, None] | self.fixed[:, None, :]] = 0
        r = np.arange(na)
        M[:, r, r] = np.where(self.fixed, dtype(1), M[:, r, r])
        self.M = M

    def product(self, x):
        """S x (x (m, na)) with zeros on the fixed rows."""
        q = np.einsum("jrc,jc->jr", self.D, x)
        np.add.at(q, self.oj, np.einsum("brc,bc->br", self.O, x[self.ok]))
        np.add.at(q, self.ok, np.einsum("brc,br->bc", self.O, x[self.oj]))
        return np.where(self.fixed, self.dtype(0), q)

    def dense(self):
        """The symmetric dense matrix with the rule applied."""
        m, na = self.m, self.na
        S = np.zeros((na * m, na * m), dtype=self.dtype)
        for j in range(m):
            S[na * j:na * j + na, na * j:na * j + na] = self.M[j]
        f = self.fixed
        for B, j, k in zip(self.O, self.oj, self.ok):
            B = np.where(f[j][:, None] | f[k][None, :], self.dtype(0), B)
            S[na * j:na * j + na, na * k:na * k + na] = B
            S[na * k:na * k + na, na * j:na * j + na] = B.T
        return S


def chol_inverse(M):
    """(M^-1 (count, na, na), ok (count,)) of a stack of symmetric blocks by
    Cholesky, in M's dtype; ok is False where a pivot was not positive (the
    inverse is then zero)."""
    M = np.asarray(M)
    n, na = M.shape[0], M.shape[1]
    dt = M.dtype.type
    L = np.zeros_like(M)
    ok = np.ones(n, dtype=bool)
    for c in range(na):
        d = M[:, c, c] - np.einsum("jk,jk->j", L[:, c, :c], L[:, c, :c])
        ok &= (d > 0) & np.isfinite(d)
        l = np.sqrt(np.where(ok, d, dt(1)))
        L[:, c, c] = l
        for i in range(c + 1, na):
            L[:, i, c] = (M[:, i, c] - np.einsum("jk,jk->j", L[:, i, :c], L[:, c, :c])) / l
    Y = np.zeros_like(M)                        # L Y = I
    for i in range(na):
        rhs = np.zeros((n, na), dtype=M.dtype)
        rhs[:, i] = 1
        rhs -= np.einsum("jk,jkc->jc", L[:, i, :i], Y[:, :i, :])
        Y[:, i, :] = rhs / L[:, i, i][:, None]
    X = np.zeros_like(M)                        # L^T X = Y
    for i in range(na - 1, -1, -1):
        rhs = Y[:, i, :] - np.einsum("jk,jkc->jc", L[:, i + 1:, i], X[:, i + 1:, :])
        X[:, i, :] = rhs / L[:, i, i][:, None]
    X = np.tril(X) + np.tril(X, -1).transpose(0, 2, 1)
    X[~ok] = 0
    return X, ok


def pcg(jk, blocks, e_, tol, max_iter):
    """dict of da (na * m,), iterations, relres (the recurrence's sqrt(rz_k /
    rz_0)), converged and status: 0, or 4 for a diagonal block whose Cholesky
    meets a non-positive pivot, p' S p <= 0 or a scalar that is not finite."""
    s = System(jk, blocks, e_)
    Mi, ok = chol_inverse(s.M)
    x = np.zeros((s.m, s.na))
    out = dict(da=x.reshape(-1), iterations=0, relres=0.0, converged=False, status=0)
    if not ok.all():
        return dict(out, status=4)
    r = s.e.copy()
    z = np.einsum("jrc,jc->jr", Mi, r)
    p = z.copy()
    rz = rz0 = float(np.sum(r * z))
    if not np.isfinite(rz0) or rz0 < 0:
        return dict(out, status=4)
    if rz0 == 0:
        return dict(out, converged=True)
    out["relres"] = 1.0
    for k in range(1, max_iter + 1):
        q = s.product(p)
        pq = float(np.sum(p * q))
        alpha = rz / pq if pq != 0 else np.inf
        if not pq > 0 or not np.isfinite(alpha):
            return dict(out, da=x.reshape(-1), status=4)
        x = x + alpha * p
        r = r - alpha * q
        z = np.einsum("jrc,jc->jr", Mi, r)
        rzn = float(np.sum(r * z))
        rel = float(np.sqrt(rzn / rz0)) if rzn >= 0 else np.nan
        out.update(da=x.reshape(-1), iterations=k, relres=rel)
        if not np.isfinite(rzn) or not np.isfinite(rel):
            return dict(out, status=4)
        if rel <= tol:
            return dict(out, converged=True)
        p = z + (rzn / rz) * p
        rz = rzn
    return out


def true_relres(jk, blocks, e_, da):
    """sqrt(r' M^-1 r / e_' M^-1 e_) with r = e_ - S da recomputed from the
    blocks in long double (rule applied: on a fixed row r = -da)."""
    s = System(jk, blocks, e_, dtype=LD)
    x = np.asarray(da, dtype=np.float64).reshape(-1, order="F").astype(LD).reshape(s.m, s.na)
    Mi, ok = chol_inverse(s.M)
    assert ok.all(), "a diagonal block is not positive definite"
    xf = np.where(s.fixed, LD(0), x)
    r = s.e - s.product(xf) - np.where(s.fixed, x, LD(0))
    num = np.sum(r * np.einsum("jrc,jc->jr", Mi, r))
    den = np.sum(s.e * np.einsum("jrc,jc->jr", Mi, s.e))
    return float(np.sqrt(num / den)) if den > 0 else (0.0 if num == 0 else np.inf)


def direct(jk, blocks, e_):
    """The solution of the system (rule applied) as a long double vector: fp64
    LAPACK solves of long double residuals (cond(S) u < 1 here, so each round
    gains digits) until the corrections stop shrinking -- at about cond(S)
    2^-64 of the solution, the accuracy a long double factorisation has too."""
    s = System(jk, blocks, e_, dtype=LD)
    S = s.dense()
    S64 = S.astype(np.float64)
    e = s.e.reshape(-1)
    x = np.zeros_like(e)
    prev = np.inf
    for _ in range(30):
        dx = np.linalg.solve(S64, (e - S @ x).astype(np.float64)).astype(LD)
        size = float(np.abs(dx).max())
        if size >= 0.5 * prev:
            return x
        x = x + dx
        prev = size
    raise AssertionError("the refinement of the direct solve did not settle")
