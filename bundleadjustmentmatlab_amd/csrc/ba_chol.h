// ba_chol.h -- the reduced solve's own state (internal to libvlgba.so): the host
// plan and everything ba_chol_setup allocates or initialises for it.  One
// ba_chol per solving context, owned by ba_chol_setup / ba_chol_free through
// ba_dev::chol (null in stage-mode contexts and after the free).  The plan is
// the one source of the solve's structure: every file reads d->chol->plan.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_chol_plan.h"

struct ba_chol {
    chol_plan plan;
    // the factor's storage: S dense, column major, leading dimension lds (the
    // plan's slds under nested dissection), lower triangle, zero outside the
    // envelope; the inverses of the diagonal Cholesky tiles; the forward solve
    double *S;
    double *linv;      // [lds/64][64*64] ([nt32][32*32] with the camera-aligned CR)
    double *ywork;     // [lds + 64]
    // tile envelope of the reduced system (64 x 64 tiles): tile row i of L is
    // non-zero only in tile columns >= plan.tfirst[i] (the profile is preserved
    // by the factorisation), so tiles left of it are never touched
    int *pan_list;     // tile rows i > k with tfirst[i] <= k, per k
    int *pan_ptr;      // [nt+1] offsets into pan_list (k_backward_all, k_env_runner)
    unsigned long long *xgran64;  // [nt][128] x_k granules of the one-launch backward
    unsigned *kflag;   // [nt] envelope factor: L_kk^-1 / y_k published (epoch fac_epoch)
    unsigned *rflag;   // [4 nt + 1] runner mode's flags + its timeout word (k_env_runner;
                       // opt-in: VLGBA_ENV_RUNNER=1)
    int *env_tiles;    // [n_env][2] (i, k) tiles inside the envelope
    int *tb_ptr, *tb_blk;  // per envelope tile, the co-visible blocks overlapping it
    // block cyclic reduction (tile-tridiagonal S): per level, eliminated tiles
    // (e, p, q) and kept tiles (k, e-, e+, k2); -1 = none
    int *cr_elim, *cr_keep;       // [3 * ne], [4 * nk]
    double *crL;                  // [2][nt][64*64] L(p, e) | L(q, e)
    // camera-aligned cyclic reduction (plan.cr32): tiles of tb32 = NA * floor(32
    // / NA) rows (whole cameras, <= 32), padded to 32 in LDS with an identity
    // block; chosen when S is tridiagonal at that granularity (half the pivot
    // chain per level of the 64-row tiles).  crL then holds [2][nt32][32*32].
    // fused levels (L >= 1): records (e, p, q, em, ep) and survivors (k, em, ep)
    int *crf, *crs;
    // one-launch back substitution (k_cr32_back_all): x of every tile as
    // 64 epoch-tagged 8-byte granules, read by the tiles of the level below
    unsigned long long *xgran;    // [nt32][64]
    // the whole CR in one launch (k_cr32_fused, plan.cr_fused): epoch flags per
    // (level, tile, role 0..2 | survivor)
    unsigned *crflag;             // [nlev][nt32][5]
    // one-level nested dissection of the envelope (plan.nd_np arcs of
    // consecutive cameras minus the separator: cameras coupled to an earlier
    // arc).  Rows: arc 0 | arc 1 | ... | separator, each part padded to whole
    // 64-row tiles.  Arcs never couple to each other, so step s factors column
    // s of every arc in ONE launch (k_factor_multi); the arcs' contribution to
    // the separator block is one SYRK (k_sep_update / k_sep_reduce), then the
    // separator's columns.
    int *nd_crow;                 // [m] first row of camera j
    int *nd_prow;                 // [lds] row of camera-space entry c (-1: padding)
    int *nd_rowsrc;               // [slds] camera-space entry of row r (-1: padding)
    double *nd_rhs, *nd_x;        // [slds] the rhs / solution in row order
    int *nd_pair;                 // [npair][2] (i, j), i >= j, ascending
    int *nd_pptr;                 // [npair + 1] records of each pair
    int *nd_rec;                  // [nrec][3] (pair, kofs, kcnt)
    int *nd_klist;                // the arc columns of the records
    double *nd_part;              // [nrec][64*64 + 64] per-record L_i L_j^T | L_i y
    unsigned fac_epoch;           // per envelope factorisation with the hand-off, never 0
    unsigned back_epoch;          // per solve with a one-launch back substitution, never 0
    // runner mode (k_env_runner): on for this context (plan.env_runner asked
    // for it; cleared for good by ba_env_runner_timed_out or a missing stream)
    int env_runner;
    int runner_runs;          // runner launches made (vlgba_plan_info [28])
    int debug_runner_fail;    // the next starts fail (vlgba_debug_force_status word 6)
    hipStream_t rstream;      // the runner's stream (the process's, highest priority)
    long long bytes;          // device memory ba_chol_setup allocated (vlgba_plan_info [32])
};
