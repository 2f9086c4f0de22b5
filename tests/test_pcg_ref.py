"""The block-Jacobi PCG's reference (tests/pcg_ref.py) and host planner
(vlgba_debug_pcg_plan, csrc/ba_chol_plan.cpp) checked on the CPU before they
judge the kernels (tests/test_gpu_pcg.py):

* on the oracle's sp_schur systems of tests/test_schur_ref.py's ladybug, cfg2-7
  and shared-64 scenes at lambda = 1e-3 the reference converges within 2000
  iterations at tolerances 1e-2, 1e-6 and 1e-8, and the residual recomputed
  from the matrix in long double (true_relres) is at most 1.01 tol: the
  recurrence's residual is the true one (the 1 % is for a different rounding of
  the same recurrences);
* da is exactly 0 on the rows of a zeroed diagonal block, a negated diagonal
  block returns the failure status;
* the planner's block CSR over both triangles equals a numpy construction on
  those block lists, on m = 1 and with a camera without any block, and refuses
  a pair with j < k and a pair given twice;
* the Python and C interfaces name the solver and its entries, at ABI 6.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import pcg_ref
import schur_ref as sr
import test_schur_ref as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ladybug", "cfg2-7", "shared-64")
TOLS = (1e-2, 1e-6, 1e-8)


@functools.lru_cache(maxsize=None)
def _system(name):
    """(jk, blocks, e_) of the oracle's system, as reduced_system(dense=False)
    returns one (shared, never modified: the tests copy what they change)."""
    c = tsr._case(name)
    jk = np.asarray(c["ref"]["jk"], dtype=np.int64)
    return jk, sr.blocks_of(c["S"], jk, c["na"]), c["e"].copy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_converges_to_the_true_residual(oracle, name):
    jk, blocks, e_ = _system(name)
    for tol in TOLS:
        out = pcg_ref.pcg(jk, blocks, e_, tol, 2000)
        true = pcg_ref.true_relres(jk, blocks, e_, out["da"])
        print(f"PCG-REF {name} tol {tol:g}: {out['iterations']} iterations, recurrence "
              f"{out['relres']:.4g}, true {true:.4g}")
        assert out["status"] == 0 and out["converged"]
        assert 1 <= out["iterations"] < 2000 and out["relres"] <= tol
        assert true <= 1.01 * tol


def test_zeroed_diagonal_block_rows_are_exactly_zero(oracle):
    jk, blocks, e_ = _system("cfg2-7")
    na, cam = blocks.shape[1], 4
    rows = slice(na * cam, na * cam + na)
    d = np.flatnonzero((jk[:, 0] == cam) & (jk[:, 1] == cam))[0]
    touching = (jk[:, 0] == cam) | (jk[:, 1] == cam)
    # the whole camera zeroed (as fix_motion or a pivot leaves it), and the
    # diagonal block alone: the rule looks at the diagonal only
    for sel in (touching, np.arange(len(jk)) == d):
        B = blocks.copy()
        B[sel] = 0.0
        out = pcg_ref.pcg(jk, B, e_, 1e-8, 2000)
        assert out["status"] == 0 and out["converged"]
        assert np.array_equal(out["da"][rows], np.zeros(na))
        assert np.abs(np.delete(out["da"], np.r_[rows])).min() > 0
        assert pcg_ref.true_relres(jk, B, e_, out["da"]) <= 1.01e-8
    # one entry of the diagonal zeroed: that row alone
    B = blocks.copy()
    B[d, 2, :] = B[d, :, 2] = 0.0
    out = pcg_ref.pcg(jk, B, e_, 1e-8, 2000)
    assert out["status"] == 0 and out["da"][na * cam + 2] == 0.0
    assert np.count_nonzero(out["da"]) == out["da"].size - 1
    # a camera whose diagonal block is missing from the list
    keep = np.arange(len(jk)) != d
    out = pcg_ref.pcg(jk[keep], blocks[keep], e_, 1e-8, 2000)
    assert out["status"] == 0 and np.array_equal(out["da"][rows], np.zeros(na))


def test_failure_status(oracle):
    jk, blocks, e_ = _system("cfg2-7")
    d = np.flatnonzero(jk[:, 0] == jk[:, 1])[3]
    B = blocks.copy()
    B[d] = -B[d]
    out = pcg_ref.pcg(jk, B, e_, 1e-8, 2000)
    assert out["status"] == 4 and not out["converged"] and out["iterations"] == 0
    # positive diagonal blocks, an indefinite matrix: p' S p <= 0 on the way
    B = blocks.copy()
    off = jk[:, 0] != jk[:, 1]
    B[off] = 50.0 * B[off]
    out = pcg_ref.pcg(jk, B, e_, 1e-8, 2000)
    assert out["status"] == 4 and not out["converged"]
    # a zero right-hand side: da = 0 without an iteration
    out = pcg_ref.pcg(jk, blocks, np.zeros_like(e_), 1e-8, 2000)
    assert out["status"] == 0 and out["converged"] and out["iterations"] == 0
    assert not out["da"].any()


def test_iteration_limit_returns_the_iterate(oracle):
    jk, blocks, e_ = _system("ladybug")
    out = pcg_ref.pcg(jk, blocks, e_, 1e-12, 3)
    assert out["status"] == 0 and not out["converged"] and out["iterations"] == 3
    assert out["relres"] > 1e-12 and np.all(np.isfinite(out["da"]))
    # every CG iterate from zero has da' (e_ - S da) = 0 up to rounding and is
    # a descent direction of the model: da' e_ = da' S da > 0
    s = pcg_ref.System(jk, blocks, e_)
    x = out["da"].reshape(s.m, s.na)
    xe, xSx = np.sum(x * s.e), np.sum(x * s.product(x))
    assert xe > 0 and abs(xe - xSx) <= 1e-10 * xe


def test_direct_is_the_solution(oracle):
    jk, blocks, e_ = _system("cfg2-7")
    x = pcg_ref.direct(jk, blocks, e_)
    c = tsr._case("cfg2-7")
    # (no fixed rows in this system: the oracle's S as it is.)  Rounded to fp64
    # entry by entry, the solution has a componentwise backward error of one
    # rounding: |S dx| <= u |S| |x|
    x64 = np.asarray(x, dtype=np.float64)
    assert sr.residual(c["S"], e_, x64) <= 2 * 2.0 ** -53
    # ... which LAPACK's own solution does not reach
    s = pcg_ref.System(jk, blocks, e_)
    lap = np.linalg.solve(s.dense(), s.e.reshape(-1))
    assert sr.residual(c["S"], e_, lap) > sr.residual(c["S"], e_, x64)


# ---- the host planner ---------------------------------------------------------
def _plan_numpy(m, jk):
    rows = [[] for _ in range(m)]
    for b, (j, k) in enumerate(np.asarray(jk).reshape(-1, 2)):
        rows[j].append((k, b, 0))
        if j != k:
            rows[k].append((j, b, 1))
    rowptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ent = [(b, t) for r in rows for _, b, t in sorted(r)]
    return rowptr, np.array(ent, dtype=np.int32).reshape(-1, 2)


def _plan_lib(m, jk):
    from bundleadjustmentmatlab_amd import _lib
    L = _lib.lib()
    jk = np.ascontiguousarray(np.asarray(jk, dtype=np.int32).reshape(-1, 2))
    nb = len(jk)
    rowptr = np.full(m + 1, -7, dtype=np.int32)
    ent = np.full((2 * max(nb, 1), 2), -7, dtype=np.int32)
    nnz = L.vlgba_debug_pcg_plan(m, jk.ctypes.data_as(_lib.c_ip), nb,
                                 rowptr.ctypes.data_as(_lib.c_ip), ent.ctypes.data_as(_lib.c_ip))
    return nnz, rowptr, ent


@pytest.mark.parametrize("name", NAMES)
def test_plan_matches_numpy_on_the_scenes(oracle, name):
    jk, _, e_ = _system(name)
    m = tsr._case(name)["sc"].m
    nnz, rowptr, ent = _plan_lib(m, jk)
    want_ptr, want_ent = _plan_numpy(m, jk)
    assert nnz == len(want_ent) == 2 * len(jk) - m      # every diagonal block is listed
    assert np.array_equal(rowptr, want_ptr) and np.array_equal(ent[:nnz], want_ent)
    assert np.all(ent[nnz:] == -7)                      # nothing written past nnz
    # a shuffled block list: the same rows, the shuffled indices
    perm = np.random.default_rng(5).permutation(len(jk))
    nnz2, rowptr2, ent2 = _plan_lib(m, jk[perm])
    want_ptr2, want_ent2 = _plan_numpy(m, jk[perm])
    assert nnz2 == nnz and np.array_equal(rowptr2, want_ptr)
    assert np.array_equal(ent2[:nnz], want_ent2)
    assert np.array_equal(perm[ent2[:nnz, 0]], ent[:nnz, 0])


def test_plan_edges():
    nnz, rowptr, ent = _plan_lib(1, [[0, 0]])
    assert nnz == 1 and rowptr.tolist() == [0, 1] and ent[0].tolist() == [0, 0]
    # camera 1 has no block at all, camera 3 no diagonal block
    jk = [[2, 0], [0, 0], [3, 2], [2, 2]]
    nnz, rowptr, ent = _plan_lib(4, jk)
    want_ptr, want_ent = _plan_numpy(4, jk)
    assert nnz == 6 and rowptr.tolist() == [0, 2, 2, 5, 6] == want_ptr.tolist()
    assert np.array_equal(ent[:nnz], want_ent)
    assert ent[:nnz].tolist() == [[1, 0], [0, 1], [0, 0], [3, 0], [2, 1], [2, 0]]
    nnz, rowptr, _ = _plan_lib(3, np.zeros((0, 2)))
    assert nnz == 0 and rowptr.tolist() == [0, 0, 0, 0]
    assert _plan_lib(3, [[0, 0], [1, 2]])[0] == -1          # j < k
    assert _plan_lib(3, [[0, 0], [2, 1], [2, 1]])[0] == -1  # a pair twice
    assert _plan_lib(3, [[0, 0], [1, 1], [1, 1]])[0] == -1
    assert _plan_lib(3, [[3, 0]])[0] == -1                  # out of range
    assert _plan_lib(3, [[1, -1]])[0] == -1
    assert _plan_lib(0, [[0, 0]])[0] == -1


def test_interface_names_the_solver():
    from bundleadjustmentmatlab_amd import _lib
    from bundleadjustmentmatlab_amd.bundle import BundleAdjuster
    assert BundleAdjuster.SOLVERS["pcg"] == 5
    assert BundleAdjuster.PLAN_KEYS[31:] == ("pcg", "solve_bytes")
    hdr = open(os.path.join(ROOT, "include", "vlgba.h")).read()
    assert re.search(r"#define\s+VLGBA_ABI_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6
    assert re.search(r"#define\s+VLGBA_NPLAN\s+33\b", hdr)
    assert re.search(r"#define\s+VLGBA_NKERNELS\s+18\b", hdr)
    flat = " ".join(hdr.split())
    for decl in ("int vlgba_set_pcg(vlgba_ctx *ctx, double tol, int max_iter);",
                 "int vlgba_get_pcg(vlgba_ctx *ctx, double *tol, int *max_iter);",
                 "int vlgba_get_pcg_stats(vlgba_ctx *ctx, int *iterations, double *relres, "
                 "int *converged, long long *total);",
                 "int vlgba_debug_pcg_plan(int m, const int *blk_jk, int nb, int *rowptr, "
                 "int *ent);"):
        assert decl in flat, decl
    L = _lib.lib()
    assert L.vlgba_set_pcg.argtypes == [ctypes.c_void_p, ctypes.c_double, ctypes.c_int]
    assert L.vlgba_get_pcg_stats.argtypes[-1] == ctypes.POINTER(ctypes.c_longlong)
    assert L.vlgba_set_pcg(None, 0.1, 10) == -1001
    assert L.vlgba_get_pcg(None, None, None) == -1001
    assert L.vlgba_get_pcg_stats(None, None, None, None, None) == -1001
