"""The extended-precision stage reference (tests/schur_ref.py) checked on the
CPU before it judges a kernel (tests/test_gpu_stage_ref.py):

* the oracle's own fp64 stages (sp_y / sp_schur / sp_update, a different
  summation order from any GPU kernel) stay inside every per-entry bound;
* the bounds have teeth: each of a list of small, realistic mistakes in S, in
  the damping or in db leaves them;
* the componentwise backward error separates a right solve (LAPACK Cholesky,
  the oracle's fixed-row Cholesky: well below ld * u) from a solve of a system
  with one 6 x 6 block missing (above 1e3 * ld * u);
* the blockwise residual (residual_blocks: no dense S) is the dense one to the
  rounding of its long double sums, and one entry of an exact solution off by
  a relative 1e-12 lifts it above ld * u.
"""
import functools

import numpy as np
import pytest

import schur_ref as sr

LAM = 1e-3
SCENES = {
    "cfg2-6": ("cfg2", dict(m=13, n=400, seed=3), 6),
    "cfg2-7": ("cfg2", dict(m=13, n=400, seed=3), 7),
    "cfg2-10": ("cfg2", dict(m=13, n=400, seed=3), 10),
    "ladybug": ("ladybug", dict(m=40, n=1500, max_track=30, radius=150.0, seed=23), 6),
    "cfg3-t10": ("cfg3", dict(m=40, n=2000, track=10, seed=6), 6),
    # tests/track_scenes.py: 64 tracks of 91..100 views through the same 90
    # cameras (blocks of 64 and more points: sums of several hundred terms), and
    # two 257-view tracks (camera sums of 257 terms more) at num_a 6 and 10
    "shared-64": ("shared", dict(C=64), 6),
    "track-257": ("planted", dict(m=260, base_n=150, seed=5,
                                  tracks=((2, 259, 1), (0, 257, 1))), 6),
    "track-257-10": ("planted", dict(m=260, base_n=150, seed=5,
                                     tracks=((2, 259, 1), (0, 257, 1))), 10),
}


def _scene(cfg, kw):
    from bundleadjustmentmatlab_amd.scene import make_config
    if cfg == "shared":
        import track_scenes as ts
        return ts.shared(**kw)[0]
    if cfg == "planted":
        import track_scenes as ts
        kw = dict(kw, tracks=[np.arange(*t) for t in kw["tracks"]])
        return ts.planted(**kw)[0]
    return make_config(cfg, **kw)


def start_params(sc, num_a):
    a = np.zeros((num_a, sc.m), order="F")
    a[0:3], a[3:6] = sc.w0, sc.T0
    if num_a == 7:
        a[6] = sc.K[0]
    elif num_a == 10:
        a[6:10] = sc.K
    return a, np.asfortranarray(sc.X0[:3])


def w_of(W, na):
    """The oracle's (N, 3 na) W as the getter's (na, 3, N)."""
    return np.asfortranarray(W.T).reshape(na, 3, -1, order="F")


@functools.lru_cache(maxsize=None)
def _case(name, lam=LAM):
    """One oracle pass of the scene at lam and the reference of its stages
    (computed once, shared, never modified: the tests copy what they change)."""
    import bundle_euclid_ref as oracle
    cfg, kw, na = SCENES[name]
    sc = _scene(cfg, kw)
    a, b = start_params(sc, na)
    pb = oracle.SparseProblem(sc.m, sc.n, sc.obs_pt, sc.obs_cam, sc.obs_x, sc.K)
    L = oracle.sp_linearize(pb, a, b, na)
    Vi = oracle.pinv3_formula(sr.damp(L["V"], lam))
    Y = oracle.sp_y(pb, L["W"], Vi, na)
    S, e_ = oracle.sp_schur(pb, Y, L["W"], sr.damp(L["U"], lam), L["eA"], L["eB"], na)
    ref = sr.schur(sc.m, sc.n, na, sc.obs_pt, sc.obs_cam, w_of(L["W"], na), L["V"], L["eB"],
                   L["U"], L["eA"], lam)
    return dict(sc=sc, na=na, a=a, b=b, pb=pb, L=L, Vi=Vi, Y=Y, S=S, e=e_.reshape(-1), ref=ref)


def _ratios(c, S, e=None):
    jk = c["ref"]["jk"]
    return sr.schur_ratio(c["ref"], jk, sr.blocks_of(S, jk, c["na"]), c["e"] if e is None else e)


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_within_bounds(oracle, name):
    c = _case(name)
    na, sc = c["na"], c["sc"]
    rs, re = _ratios(c, c["S"])
    # every block of the oracle's S outside the reference's list is zero
    full = np.zeros_like(c["S"])
    for (j, k), B in zip(c["ref"]["jk"], sr.blocks_of(c["S"], c["ref"]["jk"], na)):
        full[na * j:na * j + na, na * k:na * k + na] = B
    assert np.array_equal(np.tril(full), np.tril(c["S"]))
    da = oracle.chol_solve_fixed(c["S"], c["e"])
    out = {}
    for ndb in sorted({6, na}):
        db = oracle.sp_update(c["pb"], c["L"]["W"], da, c["L"]["eB"], c["Vi"], c["a"], c["b"],
                              na, ndb=ndb)[0]
        rdb, bnd = sr.back_subst(na, ndb, sc.obs_pt, sc.obs_cam, w_of(c["L"]["W"], na), c["Vi"],
                                 c["L"]["eB"], da)
        out[ndb] = sr.db_ratio(db, rdb, bnd)
    print(f"{name}: S {rs:.3g} e_ {re:.3g} db {out} of the bound")
    assert rs <= 1.0 and re <= 1.0 and max(out.values()) <= 1.0


def _offdiag_block(c, smallest=False):
    """An off-diagonal block (index into ref): the one with the most points,
    or the one of the smallest magnitude."""
    r = c["ref"]
    off = np.flatnonzero(r["jk"][:, 0] != r["jk"][:, 1])
    if smallest:
        mag = np.abs(r["S"][off]).max(axis=(1, 2)).astype(float)
        return off[np.argmin(np.where(mag > 0, mag, np.inf))]
    return off[np.argmax(r["npts"][off])]


@pytest.mark.parametrize("name", ["cfg2-6", "cfg2-10", "ladybug", "shared-64", "track-257"])
def test_bound_has_teeth_on_s(oracle, name):
    c = _case(name)
    na, sc, r = c["na"], c["sc"], c["ref"]
    sl = lambda j, k: (slice(na * j, na * j + na), slice(na * k, na * k + na))   # noqa: E731
    assert max(_ratios(c, c["S"])) <= 1.0
    # one point's term dropped from one off-diagonal block
    j, k = r["jk"][_offdiag_block(c)]
    pt, cam = sc.obs_pt, sc.obs_cam
    i = np.intersect1d(pt[cam == j], pt[cam == k])[0]
    oj = np.flatnonzero((pt == i) & (cam == j))[0]
    ok = np.flatnonzero((pt == i) & (cam == k))[0]
    term = c["Y"][oj].reshape(3, na).T @ c["L"]["W"][ok].reshape(3, na)
    S = c["S"].copy()
    S[sl(j, k)] += term
    assert _ratios(c, S)[0] > 1.0
    # one off-diagonal block transposed
    S = c["S"].copy()
    S[sl(j, k)] = S[sl(j, k)].T.copy()
    assert _ratios(c, S)[0] > 1.0
    # two cameras' diagonal blocks swapped
    S = c["S"].copy()
    S[sl(1, 1)], S[sl(2, 2)] = c["S"][sl(2, 2)], c["S"][sl(1, 1)]
    assert _ratios(c, S)[0] > 1.0
    # one entry of the smallest block off by 1e-10 relative
    j, k = r["jk"][_offdiag_block(c, smallest=True)]
    S = c["S"].copy()
    B = S[sl(j, k)]
    q = np.unravel_index(np.argmax(np.abs(B)), B.shape)
    B[q] *= 1 + 1e-10
    assert _ratios(c, S)[0] > 1.0
    # one entry of e_ off by 1e-10 relative
    e = c["e"].copy()
    e[np.argmax(np.abs(e))] *= 1 + 1e-10
    assert _ratios(c, c["S"], e)[1] > 1.0
    # damped with 1.1e-3 where the reference has 1e-3
    w = _case(name, 1.1e-3)
    rs, re = _ratios(c, w["S"], w["e"])
    assert rs > 1.0 and re > 1.0


def test_bound_has_teeth_on_db(oracle):
    """num_a = 10: the MEX back substitution takes six terms per observation
    (mex_bundle_3_db_new.c:113-120); all ten is the nomex twin's."""
    c = _case("cfg2-10")
    na, sc = c["na"], c["sc"]
    da = oracle.chol_solve_fixed(c["S"], c["e"])
    assert np.abs(da.reshape(na, -1, order="F")[6:]).max() > 0
    W = w_of(c["L"]["W"], na)
    db = {ndb: oracle.sp_update(c["pb"], c["L"]["W"], da, c["L"]["eB"], c["Vi"], c["a"], c["b"],
                                na, ndb=ndb)[0] for ndb in (6, na)}
    for right, wrong in ((6, na), (na, 6)):
        ref, bnd = sr.back_subst(na, right, sc.obs_pt, sc.obs_cam, W, c["Vi"], c["L"]["eB"], da)
        assert sr.db_ratio(db[right], ref, bnd) <= 1.0
        assert sr.db_ratio(db[wrong], ref, bnd) > 1.0
    # one point's db off by 1e-10 relative
    ref, bnd = sr.back_subst(na, 6, sc.obs_pt, sc.obs_cam, W, c["Vi"], c["L"]["eB"], da)
    bad = db[6].copy()
    bad[np.unravel_index(np.argmax(np.abs(bad)), bad.shape)] *= 1 + 1e-10
    assert sr.db_ratio(bad, ref, bnd) > 1.0


@pytest.mark.parametrize("name", ["track-257", "track-257-10"])
def test_bound_has_teeth_on_a_long_tracks_last_view(oracle, name):
    """A 257-view track's db without the term of its 257th observation (what a
    256-lane loop that forgot its second trip would give) leaves the bound,
    with ndb = 6 and ndb = num_a alike."""
    c = _case(name)
    na, sc = c["na"], c["sc"]
    pt, cam = sc.obs_pt, sc.obs_cam
    da = oracle.chol_solve_fixed(c["S"], c["e"])
    W = w_of(c["L"]["W"], na)
    i = sc.base_n
    last = np.flatnonzero(pt == i)[-1]
    assert (pt == i).sum() == 257
    for ndb in sorted({6, na}):
        db = oracle.sp_update(c["pb"], c["L"]["W"], da, c["L"]["eB"], c["Vi"], c["a"], c["b"],
                              na, ndb=ndb)[0]
        ref, bnd = sr.back_subst(na, ndb, pt, cam, W, c["Vi"], c["L"]["eB"], da)
        assert sr.db_ratio(db, ref, bnd) <= 1.0
        term = W[:ndb, :, last].T @ da.reshape(na, -1, order="F")[:ndb, cam[last]]
        bad = db.copy()
        bad[:, i] += c["Vi"][:, :, i] @ term
        assert sr.db_ratio(bad, ref, bnd) > 1.0, ndb


@pytest.mark.parametrize("name", ["cfg2-6", "cfg2-10", "ladybug", "cfg3-t10"])
def test_residual_separates_right_from_wrong(oracle, name):
    import scipy.linalg as sl
    c = _case(name)
    na = c["na"]
    S, e = c["S"], c["e"]
    ld = S.shape[0]
    bar = ld * sr.U53
    Ssym = sr.symmetrise(S)
    x_lapack = sl.cho_solve(sl.cho_factor(Ssym, lower=True), e)
    x_fixed = oracle.chol_solve_fixed(S, e)
    eta = [sr.residual(np.tril(S), e, x) for x in (x_lapack, x_fixed)]
    print(f"{name}: ld {ld} cond {np.linalg.cond(Ssym):.2g} eta / (ld u) "
          f"{eta[0] / bar:.3g} {eta[1] / bar:.3g}")
    assert max(eta) <= bar
    # the same solves of a system with one 6 x 6 block (and its mirror) zeroed
    j, k = c["ref"]["jk"][_offdiag_block(c)]
    Sb = Ssym.copy()
    Sb[na * j:na * j + 6, na * k:na * k + 6] = 0.0
    Sb[na * k:na * k + 6, na * j:na * j + 6] = 0.0
    xb = np.linalg.solve(Sb, e)      # (no longer positive definite in general)
    assert sr.residual(np.tril(S), e, xb) > 1e3 * bar


def test_residual_rows_and_exact_zeros():
    """Fixed rows (zero row of S, zero e_, zero da) count as satisfied; a
    non-zero residual over a zero denominator does not."""
    S = np.diag([2.0, 0.0, 4.0])
    assert sr.residual(S, [2.0, 0.0, 4.0], [1.0, 0.0, 1.0]) == 0.0
    assert sr.residual(S, [2.0, 0.0, 4.0], [1.0, 0.0, 2.0]) > 0.1
    assert sr.residual(S, [2.0, 0.0, 4.0], [1.0, 0.0, 2.0], rows=np.array([1, 1, 0], bool)) == 0.0
    assert sr.residual(np.zeros((1, 1)), [0.0], [0.0]) == 0.0


def _banded_blocks(m, na, track, seed, integers=False):
    """A random block-banded system as the getter returns one: every pair
    j >= k with j - k < track once, in shuffled order; the strict upper triangle
    of a diagonal block is junk that nobody may read.  integers: entries that
    are multiples of 2^-10 below 16, the diagonal dominant."""
    rng = np.random.default_rng(seed)
    jk = np.array([(j, k) for j in range(m) for k in range(max(0, j - track + 1), j + 1)])
    jk = jk[rng.permutation(len(jk))]
    if integers:
        blocks = rng.integers(-(1 << 13), 1 << 13, (len(jk), na, na)) / 1024.0
    else:
        blocks = rng.standard_normal((len(jk), na, na))
        blocks *= 10.0 ** rng.integers(-3, 4, (len(jk), 1, 1))
    for b in np.flatnonzero(jk[:, 0] == jk[:, 1]):
        blocks[b] += np.triu(np.full((na, na), 1e300), 1)
        if integers:
            blocks[b][np.diag_indices(na)] = float(1 << 12) + rng.integers(0, 64, na)
    return jk, blocks


def _dense_lower(m, na, jk, blocks):
    """The dense S of tests/test_gpu_stage_ref.py::test_solve_stage."""
    S = np.zeros((na * m, na * m))
    for (j, k), B in zip(jk, blocks):
        S[na * j:na * j + na, na * k:na * k + na] = np.tril(B) if j == k else B
    return S


@pytest.mark.parametrize("m,na,track", [(23, 6, 9), (17, 9, 6), (11, 12, 5), (5, 7, 1)])
def test_residual_blocks_is_the_dense_residual(m, na, track):
    """residual_blocks against residual on the dense S test_solve_stage
    builds, with a row mask, an unobserved camera (zero rows and columns, zero
    e_ and da: 0 / 0 counts as satisfied).  Not to the
    last bit: a row's terms are added block by block and not column by column,
    so each sum carries its own rounding -- within residual_slack of each
    other, which is below 1e-2 of ld * u here.  da is an fp64 solve of the
    system, so eta is the small number it is in use."""
    rng = np.random.default_rng(m)
    jk, blocks = _banded_blocks(m, na, track, seed=na)
    ld = na * m
    e = rng.standard_normal(ld)
    dead = m // 2
    blocks[(jk[:, 0] == dead) | (jk[:, 1] == dead)] = 0.0
    e[na * dead:na * dead + na] = 0.0
    Sfull = sr.symmetrise(_dense_lower(m, na, jk, blocks))
    live = np.repeat(np.arange(m) != dead, na)
    x = np.zeros(ld)
    x[live] = np.linalg.solve(Sfull[np.ix_(live, live)], e[live])
    da = np.asfortranarray(x.reshape(na, m, order="F"))
    rows = rng.random(ld) < 0.8
    rows[na * dead:na * dead + na] = True
    S = _dense_lower(m, na, jk, blocks)
    terms = na * (2 * track - 1)
    for mask in (None, rows, np.zeros(ld, bool)):
        want, got = sr.residual(S, e, da, mask), sr.residual_blocks(m, na, jk, blocks, e, da, mask)
        slack = sr.residual_slack(terms, want)
        print(f"m {m} na {na} track {track}: dense {want:.17g} blocks {got:.17g} "
              f"slack {slack:.3g} = {slack / (ld * sr.U53):.3g} ld u")
        assert np.isfinite(want) and abs(got - want) <= slack
        assert want < 1e-6 and slack <= 1e-2 * ld * sr.U53
    assert sr.residual_blocks(m, na, jk, blocks, e, da, np.zeros(ld, bool)) == 0.0
    # a right-hand side on a row with nothing in it is a whole miss, in both
    e[na * dead] = 1.0
    assert sr.residual(S, e, da) == 1.0 == sr.residual_blocks(m, na, jk, blocks, e, da)
    # the small cases of test_residual_rows_and_exact_zeros
    one = np.array([[0, 0], [1, 1], [2, 2]]), np.array([2.0, 0.0, 4.0]).reshape(3, 1, 1)
    assert sr.residual_blocks(3, 1, *one, [2.0, 0.0, 4.0], [1.0, 0.0, 1.0]) == 0.0
    assert sr.residual_blocks(3, 1, *one, [2.0, 0.0, 4.0], [1.0, 0.0, 2.0]) > 0.1
    assert sr.residual_blocks(3, 1, *one, [2.0, 0.0, 4.0], [1.0, 0.0, 2.0],
                              rows=np.array([1, 1, 0], bool)) == 0.0


@pytest.mark.parametrize("m,na,track", [(23, 6, 9), (11, 12, 5)])
def test_residual_blocks_notices_one_entry(m, na, track):
    """An exact solution: S in multiples of 2^-10 below 2^13, x integers below
    2^10, so e_ = S x is exact in fp64 (every product and partial sum fits 53
    bits) and both residuals are exactly zero.  One entry of x off by a relative
    1e-12 lifts row r to |S_rr x_r| 1e-12 / (|S||x| + |e_|)_r on the dominant
    diagonal: 4096 <= |S_rr| < 4160, the row's other entries (at most 131, each
    at most 8) sum to 1048 at the most and 512 <= |x| < 1024, so the quotient is
    at least 4096 * 512 / (2 * 5208 * 1024) = 0.19 -- eta >= 1.9e-13 against
    ld * u = 1.5e-14."""
    rng = np.random.default_rng(7)
    jk, blocks = _banded_blocks(m, na, track, seed=1, integers=True)
    ld = na * m
    S = _dense_lower(m, na, jk, blocks)
    x = rng.integers(512, 1024, ld).astype(np.float64) * rng.choice([-1.0, 1.0], ld)
    e = sr.symmetrise(S) @ x
    assert np.array_equal(e.astype(sr.LD), sr.symmetrise(S).astype(sr.LD) @ x.astype(sr.LD))
    da = np.asfortranarray(x.reshape(na, m, order="F"))
    assert sr.residual_blocks(m, na, jk, blocks, e, da) == 0.0 == sr.residual(S, e, da)
    bar = ld * sr.U53
    for r in (0, ld // 2 + 1, ld - 1):
        bad = x.copy()
        bad[r] *= 1 + 1e-12
        bad = bad.reshape(na, m, order="F")
        eta = sr.residual_blocks(m, na, jk, blocks, e, bad)
        print(f"m {m} na {na}: row {r} off by 1e-12: eta / (ld u) {eta / bar:.3g}")
        assert eta > bar and eta >= 1.9e-13
        assert abs(eta - sr.residual(S, e, bad)) <= sr.residual_slack(na * (2 * track - 1), eta)
        # ... and a mask that leaves out every row the entry couples to does not see it
        j = r // na
        far = np.repeat(np.abs(np.arange(m) - j) >= track, na)
        assert sr.residual_blocks(m, na, jk, blocks, e, bad, far) == 0.0


# ---------------------------------------------------------------------------
# num_a = 9 (the radial camera): the oracle has no such camera, so W, V, eB, U,
# eA come from tests/radial_ref.py and the fp64 stage is restated here
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _radial_case():
    """A banded scene of 9 cameras and 60 points in tracks of 4 under the lens
    (tests/test_gpu_stage_ref.py::_radial's start and observations): the
    reference of its Schur stage and a dense fp64 restatement of S and e_."""
    import radial_ref as ra
    from bundleadjustmentmatlab_amd.scene import make_config
    na = 9
    sc = make_config("cfg2", m=9, n=60, track=4, seed=3)
    pt, cam, m, n = sc.obs_pt, sc.obs_cam, sc.m, sc.n
    kt = np.tile(np.array(ra.K_TRUE)[:, None], (1, m))
    ox = ra.observe(sc.K, ra.pack(sc.K, sc.w, sc.T, kt), sc.X, pt, cam, 0.5, 77)
    a = ra.pack(sc.K, sc.w0, sc.T0, kt * np.array([[0.9], [1.2]]))
    b = np.asfortranarray(sc.X0[:3])
    e = np.asarray(ra.residuals(sc.K, a, b, pt, cam, ox)[0], dtype=np.float64)
    R = ra.linearization(sc.K, a, b, pt, cam, e, m, n)
    L = {k: np.asfortranarray(np.asarray(R[k], dtype=np.float64))
         for k in ("U", "eA", "V", "eB", "W")}
    assert L["W"].shape == (na, 3, len(pt)) and L["U"].shape == (na, na, m)
    ref = sr.schur(m, n, na, pt, cam, L["W"], L["V"], L["eB"], L["U"], L["eA"], LAM)
    # fp64, dense, another order than any kernel's: Y = W V*^-1 per observation,
    # S = U* - Y W^T over the whole 81 x 180 matrices, e_ = eA - Y eB
    Vi = sr.vinv_of(L["V"], LAM)
    Wo = L["W"].transpose(2, 0, 1)                                   # (N, na, 3)
    Yo = np.einsum("orq,oqc->orc", Wo, Vi.transpose(2, 0, 1)[pt])
    Wd, Yd = np.zeros((na * m, n, 3)), np.zeros((na * m, n, 3))
    rows = na * cam[:, None] + np.arange(na)[None, :]
    Wd[rows, pt[:, None], :] = Wo
    Yd[rows, pt[:, None], :] = Yo
    S = -Yd.reshape(na * m, 3 * n) @ Wd.reshape(na * m, 3 * n).T
    Us = sr.damp(L["U"], LAM)
    for j in range(m):
        S[na * j:na * j + na, na * j:na * j + na] += Us[:, :, j]
    e_ = L["eA"].reshape(-1, order="F") - Yd.reshape(na * m, 3 * n) @ L["eB"].T.reshape(-1)
    return dict(sc=sc, na=na, L=L, ref=ref, S=S, e=e_, Yo=Yo, Wo=Wo)


def test_radial_restatement_within_bounds_and_teeth():
    """num_a = 9: an fp64 restatement of S and e_ from radial_ref's W, V, eB, U,
    eA lies within the per-entry bounds; one dropped term leaves them, and so
    does an entry moved by eight ulps of its block's largest term -- in the
    block with the most points, and in a block that straddles a 16-row tile
    boundary of k_schur_mfma's slab (the second camera of a chunk: slab rows
    9 .. 17; the entry moved is its last row's, slab row 17)."""
    c = _radial_case()
    na, sc, r = c["na"], c["sc"], c["ref"]
    pt, cam = sc.obs_pt, sc.obs_cam
    sl = lambda j, k: (slice(na * j, na * j + na), slice(na * k, na * k + na))   # noqa: E731
    rs, re = _ratios(c, c["S"])
    print(f"radial9: S {rs:.3g} e_ {re:.3g} of the bound")
    assert rs <= 1.0 and re <= 1.0
    assert np.all(np.abs(c["L"]["W"][6:9]).max(axis=(1, 2)) > 0)

    def terms(j, k):     # the block's terms, one (na, na) per point that sees both
        both = np.intersect1d(pt[cam == j], pt[cam == k])
        oj = [np.flatnonzero((pt == i) & (cam == j))[0] for i in both]
        ok = [np.flatnonzero((pt == i) & (cam == k))[0] for i in both]
        return np.einsum("prq,pcq->prc", c["Yo"][oj], c["Wo"][ok])

    j, k = r["jk"][_offdiag_block(c)]
    # one point's term dropped from the block with the most points
    S = c["S"].copy()
    S[sl(j, k)] += terms(j, k)[0]
    assert _ratios(c, S)[0] > 1.0
    # one observation's term dropped from e_
    o = np.flatnonzero(cam == j)[0]
    e = c["e"].copy()
    e[na * j:na * j + na] += c["Yo"][o] @ c["L"]["eB"][:, pt[o]]
    assert _ratios(c, c["S"], e)[1] > 1.0
    # eight ulps of the block's largest term, on the entry of the smallest
    # bound of that block ...
    bnd = np.asarray(r["bound"][_offdiag_block(c)], dtype=np.float64)
    q = np.unravel_index(np.argmin(np.where(bnd > 0, bnd, np.inf)), bnd.shape)
    S = c["S"].copy()
    S[sl(j, k)][q] += 8 * np.spacing(np.abs(terms(j, k)).max())
    assert _ratios(c, S)[0] > 1.0
    # ... and in the blocks of the second camera of a four-camera track, slab
    # rows 9 .. 17: they straddle the tile boundary 15 | 16.  The entry is in
    # the camera's k2 row (slab row 17, the second tile), whose terms f r2^2 n
    # are the block's smallest by r2^2 against the rotation and translation rows
    j0 = int(cam[0])
    assert tuple(cam[:4]) == (j0, j0 + 1, j0 + 2, j0 + 3) and na * 1 < 16 < na * 2
    T = terms(j0 + 1, j0)
    col = int(np.argmin(np.abs(T).sum(0)[8]))
    S = c["S"].copy()
    S[sl(j0 + 1, j0)][8, col] += 8 * np.spacing(np.abs(T).max())
    moved = _ratios(c, S)[0]
    print(f"radial9: slab row 17, block ({j0 + 1}, {j0}) column {col}: {moved:.3g} of the bound")
    assert moved > 1.0, moved
