// ba_chol_plan.h -- the reduced solve's host planner (ba_chol_plan.cpp): the
// 64-row tile envelope of S, the choice between camera-aligned 32-row cyclic
// reduction (CR), 64-row CR, the natural envelope and one-level nested
// dissection (ND), the records and lists each of them uploads, the solve's
// algorithmic flops and the launch plans that are passed to kernels by value.
// Host only: no HIP, RCCL or rocSOLVER header, so the planner builds with any
// C++17 compiler (tools/bench_chol_plan.cpp hashes its plans,
// tests/test_solve_plan.py pins them, tests/test_plan_sanitize.py runs it under
// the sanitizers).  ba_chol_setup (ba_chol.hip) reads the options, calls
// chol_plan_build and uploads what it returns; ba_chol_solve launches from it.
#pragma once
#include "ba_limits.h"

#include <vector>

// internal to libvlgba.so: not part of its exported ABI (vlgba_debug_nd_plan,
// declared in vlgba.h, is the planner's one exported entry)
#pragma GCC visibility push(hidden)

// ---- launch plans (plain structs, kernel arguments by value) --------------
// k_cr32_fused: the block ranges of the one-launch cyclic reduction
struct cr32_fplan {
    int nl, nrec;
    int l0two;                     // level 0 in 2 records per tile (roles 4 | 2), else 3
    int b0[BA_CR_MAXLEV + 2];      // first block of level L; b0[nl] = first back block
    int fofs[BA_CR_MAXLEV + 1];    // level L >= 1: first fused record in crf
    int sofs[BA_CR_MAXLEV + 1];    //               first survivor record in crs
    int eofs[BA_CR_MAXLEV + 2];    // elimination records of level L in cr_elim
};

// k_factor_multi: one step of the nested dissection's arcs, arc t in
// workgroups [b0[t], b0[t+1]) (k_factor_step's roles), pan / prev as offsets
// into the panel list
// Workgroup order (grouped, the default): every arc's workgroup 0 first, then
// every arc's panel tiles, then every arc's trailing pairs (pb / tb: prefix
// counts of the panels / trailing pairs over the arcs).  Arc-major order
// (b0, VLGBA_ND_GROUPED=0) puts arc 1's workgroup 0 behind all of arc 0's
// trailing pairs: once those outnumber the free workgroup slots, arc 1's
// diagonal factor -- the chain of its step -- starts only when the first of
// them retire.  The roles are the same either way (bit-identical).
struct nd_step {
    int np, grouped;
    int k[BA_ND_MAX], T[BA_ND_MAX], Tp[BA_ND_MAX], pofs[BA_ND_MAX], qofs[BA_ND_MAX];
    int ntr[BA_ND_MAX], ts[BA_ND_MAX];   // trailing pairs / their workgroups (stride)
    int kend[BA_ND_MAX];                 // runner mode: arc t's end column (else 0)
    int b0[BA_ND_MAX + 1], pb[BA_ND_MAX + 1], tb[BA_ND_MAX + 1];
};

// k_env_runner: the runs of columns [k0[t], k1[t]), one persistent workgroup each
struct env_runs {
    int np;
    int k0[BA_ND_MAX], k1[BA_ND_MAX];
};

// ---- the planner ------------------------------------------------------------
// Per-context options (ba_chol_setup reads them from the environment)
struct chol_plan_opts {
    bool cr_fused_allowed;   // one-launch CR (k_cr32_fused) unless VLGBA_CR_FUSED=0
    bool nd_off;             // VLGBA_ND=0: auto mode keeps the natural order
    bool nd_verbose;         // VLGBA_ND=v: the ND decision on stderr
    bool nd_grouped;         // k_factor_multi's workgroups by role unless VLGBA_ND_GROUPED=0
    bool env_runner;         // VLGBA_ENV_RUNNER=1: runner mode (k_env_runner)
};

struct chol_plan_in {
    int m, na;            // cameras, parameters per camera
    long long ld, lds;    // na * m, and rounded up to the 64-row tile
    int ncu;              // the device's compute units
    int dense_solve;      // ba_dev::dense_solve (0 auto .. 4 ND)
    const int *blk_jk;    // [nb][2] co-visible blocks (j >= k)
    int nb;
    chol_plan_opts opt;
};

struct chol_plan {
    // 64-row tile envelope (of the ND row order when nd_np > 0)
    int nt = 0;
    std::vector<int> tfirst;              // [nt] first envelope tile of row i
    std::vector<int> pan_ptr, pan_list;   // [nt+1], tile rows i > k inside the envelope per k
    std::vector<int> env;                 // [n_env][2] (i, k)
    std::vector<int> tptr, tblk;          // per envelope tile the co-visible blocks on it
    // cyclic reduction: per level eliminated (e, p, q) and kept (k, e-, e+, k2) tiles
    int cr32 = 0, tb32 = 0, nt32 = 0, cr_nlev = 0, asm_direct_ok = 0;
    std::vector<int> elim, keep, eptr, kptr;
    // 32-row CR: the fused levels' records (e, p, q, em, ep) / survivors (k, em, ep)
    std::vector<int> frec, srec, fptr, sptr;   // fptr / sptr [nlev+1], level 0 empty
    int cr_fused = 0;
    cr32_fplan fplan{};                        // when cr_fused
    // nested dissection
    int nd_np = 0, nd_grouped = 0;
    int nd_a0[BA_ND_MAX + 1] = {};
    long long slds = 0;
    std::vector<int> crow, prow, rowsrc;       // [m], [lds], [slds]
    std::vector<int> pairs, pptr, rec, klist;  // separator pairs and their arc-column chunks
    int nd_npair = 0, nd_nrec = 0;
    // algorithmic flops of one solve (bench.py's roofline of the solve kernels):
    // tile-dense potrf + trtri of the diagonal tiles, panel / trailing / fill /
    // SYRK GEMMs and the triangular GEMVs, each counted once (the redundant
    // factorisations of the role-split records are not).  fl_factor: the
    // launches timed as k_factor_step / k_cr_factor (with the one-launch CR its
    // back substitution too); fl_syrk: k_sep_update / k_sep_reduce; fl_back:
    // k_backward(_all) / the per-level CR back launches
    double fl_factor = 0.0, fl_syrk = 0.0, fl_back = 0.0;
    // what the setup allocates besides the lists
    bool back_one_launch = false;   // every column co-resident: pan_ptr + xgran64
    bool handoff = false;           // the envelope factor's in-launch hand-off: kflag
    int env_runner = 0;             // runner mode asked for (with the hand-off)
    bool runner_flags = false;      // ... and its flags are allocated (rflag)

    int n_env() const { return (int)env.size() / 2; }
    int cr_tiles() const { return cr32 ? nt32 : nt; }   // the CR's tile count
};

// A function of its arguments only.  Returns 0.
int chol_plan_build(const chol_plan_in &in, chol_plan &out);
// The selected inverse on the CR factors (k_cr32_selinv, ba_chol.hip) walks the
// elimination records back down; record i = (e, p, q) with both neighbours
// needs Sigma_qp, which the record of whichever of p, q was eliminated first
// (the lower level above e's) holds, since the other is its neighbour there:
// src[2 i] = that record, src[2 i + 1] = 1 when it is p's (Sigma_qp = Xq[p]^T),
// 0 when it is q's (Sigma_qp = Xp[q]); src[2 i] = -1 where p or q is absent.
// A function of elim / eptr alone.  Returns 0, or -1 for lists that are not a
// cyclic reduction's (a neighbour never eliminated, or not the source's).
int chol_selinv_sources(const std::vector<int> &elim, const std::vector<int> &eptr,
                        std::vector<int> &src);
// Step st of the ND arcs' side-by-side factorization (run: the runner started)
void chol_nd_step(const chol_plan &plan, int st, bool run, nd_step *P);

// ---- the block-Jacobi PCG's structure (ba_pcg.hip) ---------------------------
// S as a block CSR over both triangles, from the blocks the Schur phase stores
// (j >= k only): row j lists its neighbour cameras k ascending, the diagonal
// block among them, each as the block's index and whether the row reads it
// transposed (S_jk = S_kj^T for j < k).  A camera without a block has an empty
// row.
struct pcg_plan {
    std::vector<int> rowptr;   // [m + 1]
    std::vector<int> ent;      // [nnz][2] (block, transposed)
    std::vector<int> nbr;      // [nnz] the neighbour camera
    std::vector<int> dblk;     // [m] the diagonal block of camera j, or -1
};
// A function of its arguments only.  Returns nnz, or -1 for a pair with j < k,
// an index outside [0, m) or a pair given twice (vlgba_debug_pcg_plan is its
// exported entry).
int pcg_plan_build(int m, const int *blk_jk, int nb, pcg_plan &out);

#pragma GCC visibility pop
