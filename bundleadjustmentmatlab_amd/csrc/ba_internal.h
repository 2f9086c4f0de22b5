// ba_internal.h -- device-side data layout and kernel launchers of libvlgba.
//
// One ba_dev per (problem, GPU).  Everything lives in HBM for the whole solve;
// only scalars cross PCIe per LM iteration.  Layout (N = visible observations,
// NA = num_a = 6 / 7 / 10 Euclidean camera parameters, 9 with radial distortion,
// or 12 for the projective camera P(:) of bundle_projective.m, m cameras, n
// points):
//
//   observations, point-major (points ascending, cameras ascending inside a
//   point = the reference's column-major (i + n*j) visiting order per point):
//     obs_cam[N] int32, obs_x[N][2] f64, pt_ptr[n+1] int32
//   camera-major view:  cam_ptr[m+1], cam_obs[N] (obs ids ascending)
//   per observation:    jrec[N][JS]   A (2 x NA, column major) then e (2)
//                       W[N][3*NA], Y[N][3*NA]  (NA x 3 column major, as W_ij)
//                       t[N][NA]      Y_o * eB_i (the e_ contribution)
//   per camera:         a[NA*m], a_new, K4[4*m], rot[m][5][9], rot_new[m][5][9],
//                       U[NA*NA*m], eA[NA*m]
//   per point:          b[3n], b_new, V[9n], eB[3n], Vinv[9n], db[3n]
//   reduced system:     blocks (j >= k) with co-visibility: blk_jk[nb][2],
//                       blk_ptr[nb+1], term[T][2] (obs pair, point ascending),
//                       sblk[nb][NA*NA], dense S (NA*m)^2 column major, rhs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
// the chunk / group / long-track limits (BA_CH_*, BA_G*, BA_MF_*, BA_LONG_*,
// BA_LCAM_LDS, BA_LMATCH_BATCH) and the reduced solve's (BA_TILE*, BA_ND_*,
// BA_CR_MAXLEV): shared with the host planners
#include "ba_limits.h"

struct ba_chol;   // the reduced solve's state (ba_chol.h)
struct ba_pcg;    // ... of the block-Jacobi PCG (ba_pcg.h)

#define VLGBA_CHECK(x)                                                              \
    do {                                                                            \
        hipError_t err__ = (x);                                                     \
        if (err__ != hipSuccess) return -(int)err__;                                \
    } while (0)

// Per-kernel HIP-event timing (diagnostic passes only): every launch of a
// tracked kernel is bracketed by two events on the library stream; after the
// pass the elapsed times are summed per kernel.
enum {
    KT_ROT, KT_LIN, KT_CAMRED, KT_DAMP, KT_SCHUR, KT_SCHUR_CHUNK, KT_SCHUR_RED,
    KT_ASSEMBLE, KT_FACTOR, KT_SYRK, KT_BACKWARD, KT_CAMUPD, KT_PTUPD, KT_CR_FACTOR,
    KT_CR_UPDATE, KT_CR_BACK, KT_SCHUR_MF, KT_LIN_UPD, KT_N
};
#define KT_MAX_EV 8192
struct ba_ktimer {
    int on;
    int nev;
    int ncreated;      // events created so far (on first use: a context that times
                       // few launches creates few)
    hipEvent_t ev[KT_MAX_EV];
    int kid[KT_MAX_EV / 2];
    double ms[KT_N];
    long long calls[KT_N];
    double flops[KT_N];   // the reduced solve's algorithmic flops of the timed passes
};
void kt_begin(struct ba_ktimer *t, hipStream_t s);
void kt_end(struct ba_ktimer *t, hipStream_t s, int kid);

// camera model: NA == BA_PROJ_NA is the projective camera (a = P(:), 3 x 4,
// bundle_projective.m:70-73, projection mex_bundle_proj_1_XABeUVWeAeB.c:13-32;
// no K, no rotations); NA = 6 / 7 / 10 the Euclidean [w; T; (K)]
#define BA_PROJ_NA 12
// NA == BA_RAD_NA: the Euclidean camera with radial distortion, a = [w; T; f;
// k1; k2] (vlg_project_radial; analytic Jacobians only, fast path only)
#define BA_RAD_NA 9

struct ba_flags {
    int fix_structure;  // V, W, eB = 0       (bundle_euclid.m:140-144)
    int fix_motion;     // U, W, eA = 0       (:145-149)
    int has_pivot;      // pivot[m] mask      (:150-154)
};

// robust loss of the fast path and the batched one-block entries
// (vlgba_set_loss, vlgba_resect_ex; vlg_loss in vlg_math.h):
// kind 0 none, 1 Huber, 2 Cauchy; c the scale in pixels
struct ba_loss {
    int kind;
    double c;
};

// the fast path's camera reduction's arguments (ba_camred_args): to
// k_camera_reduce_chunks, or to the workgroups a pass appends to its MFMA Schur
// launch (ba_launch_schur_fast's fold: every plan with MFMA groups)
struct ba_camred {
    const int *cam_eptr, *cam_eslots;
    const double *upart;
    int m;
    ba_flags f;
    const unsigned char *pivot;
    double *U, *eA;
    const double *chsse;
    int nch;
    double *sse_out, *sse_out2;
};

// What persists for the whole solve, and nothing else: no field is written by
// one launcher in order to be read by a later one.  What one launch of a pass
// leaves for another travels as arguments and results of the launchers
// (ba_launch_schur_fast's fold and side_camred, ba_chol_solve's cam_updated,
// ba_launch_update's publish / published) and lives in locals of the pass.
struct ba_dev {
    int m, n, na, N, js;
    int device, ncu;   // HIP device ordinal and its CU count
    // problem (read-only)
    int *obs_cam, *pt_ptr, *cam_ptr, *cam_obs;
    double *obs_x, *K4;
    unsigned char *pivot;
    // state
    double *a, *b, *a_new, *b_new;
    double *rot, *rot_new;
    // linearisation
    double *jrec, *W, *U, *eA, *V, *eB;
    // per damping
    double *Vinv, *Y, *t, *db;
    // reduced system
    int nb;            // blocks
    long long T;       // terms
    int *blk_jk, *blk_ptr, *term;
    double *sblk, *rhs, *da;
    long long ld;      // NA*m
    long long lds;     // ld rounded up to the Cholesky tile (padding rows = identity)
    // the reduced solve (ba_chol.h): its plan, the dense S and its factors, the
    // lists and flags of the method the plan chose.  Owned by ba_chol_setup /
    // ba_chol_free; null in stage-mode contexts (which solve nothing)
    ba_chol *chol;
    // dense_solve = 5: block-Jacobi PCG on sblk / rhs themselves (ba_pcg.hip).
    // Owned by ba_pcg_setup / ba_pcg_free; such a context has no chol (no dense
    // S, no plan of the direct solves), every other context no pcg
    ba_pcg *pcg;
    int dense_solve;   // 0 auto, 1: every lower tile (measurement), 2: envelope, no CR,
                       // 3: sequential Cholesky (parity mode), 4: nested dissection
                       // whenever the cameras split (tests; 0 takes it when it pays),
                       // 5: block-Jacobi PCG (opt-in)
    // the two decisions a pass takes from the plan (ctx_setup):
    // direct assembly (camera-aligned CR, one rank, fast path): k_schur_reduce
    // writes each block's lower entries straight into S (and the pinv rule
    // of exactly-zero diagonals), so no k_assemble_tiles launch.  Needs every
    // lower entry of every diagonal CR tile covered by a block (the plan's
    // asm_direct_ok): the CR writes only those tiles, so S's other entries
    // keep the zeros of the setup.
    int asm_direct;
    // camera update inside the one-launch CR (k_cr32_fused, x = da in camera
    // order, a tile = whole cameras): each back record forms a_new = a + da
    // and the rotation table of its own cameras from x_e in LDS, and the
    // update's final sums (k_sum_parts3) form the camera part of dp'(lambda dp
    // + g).  camupd_fold: allowed (setup; VLGBA_CAMUPD_FOLD=0: off).  A solve
    // that did it says so (ba_chol_solve's cam_updated), and the pass hands
    // that to its update (ba_launch_update), which then launches no
    // k_camera_update.
    int camupd_fold;
    // reductions: partial sums per block of the reducing kernels, in fixed order
    double *part;      // [3][PART_MAX]
    double *scal;      // [8] : 0 old_sse, 1 new_sse, 2 dpg cams, 3 dpg pts, 4 non-positive
                       // pivot, 5 hand-off spin timeout (the solve's status words)
    // ---- fast (chunked) Schur path: points in chunks of <= CH_OBS observations;
    // per chunk the co-visible blocks it touches ("slots") and the cameras it
    // sees ("e-slots") get one partial each, reduced per block in chunk order.
    int ordered;       // 1: sequential bit-exact kernels (k_damp_point + k_schur)
    int parity;        // ordered = 2: + sequential solve and LM scalars (bit-identical
                       // LM trajectory with the oracle)
    int mfma;          // fast path: 1 = some MFMA Schur chunks (k_schur_mfma: groups
                       // [0, ngrp_mf)), 0 = term lists only (k_schur_group)
    int no_mfma;       // option: force the term-list Schur kernel
    // robust loss (fast path only): the kernels' LOSS = true instantiations run
    // when loss_kind != 0, else the plain ones
    int loss_kind;
    double loss_scale;
    // Jacobians of the fast-path linearisation (vlgba_set_jacobian): 0 the
    // reference's forward differences, 1 closed form -- rot / rot_new then hold
    // R(w), dR/dw_k, 0 per camera (rotation_k_jac) and the linearisation
    // kernels' JAC instantiations run, k_camera_update_jac / k_cr32_fused<true>
    // build the table of a_new.
    int jac;
    int ndb;           // camera parameters in the back substitution: 6 (MEX, App. A
                       // Q3) or NA (bundle_euclid_nomex.m semantics)
    int nch;           // chunks
    int *ch_pt;        // [nch+1] local point ranges
    // (the per-chunk slot / term lists stay on the host: they are folded into
    // the chunk records of `blob` and the group-slot lists below)
    int *ch_eslot;     // [nch+1] e-slot ranges
    int *eslot_optr;   // [nes+1]
    unsigned short *eslot_obs;  // [neo] chunk-local obs indices
    int *cam_eptr, *cam_eslots; // per camera: its e-slots in chunk order
    double *spart;     // [ngs][NA*NA] per group slot
    double *epart;     // [nge][NA] per group e-slot
    double *upart;     // [nes][NA(NA+1)/2 + NA] per-chunk U_j (lower) | eA_j partials
    double *chsse;     // [3][nch] per-chunk partials: linearisation SSE, new SSE, point dpg
    // fused update (fast path, ba_launch_update -> k_update_linearize): the
    // next linearisation's buffers, swapped in by an accepted step
    int fused;
    double *W2, *V2, *eB2, *upart2, *chsse2;
    int ns, nes;
    int ch_max_terms, ch_max_slots;   // per-chunk maxima: LDS staging of the term lists
    long long nterm_fast;             // (obs, obs) Schur terms of the chunk plan
    long long blob_words;             // metadata words of the chunk plan
    // Schur groups (consecutive chunks, one workgroup): block / camera partials
    // accumulate in LDS over the group's chunks and are written once per group
    int ngrp, ngs, nge;
    int grp_max_s, grp_max_e;         // LDS accumulator sizes (largest non-direct group)
    unsigned *blob;                   // per-chunk metadata records (see build_plan)
    int *ch_blob, *ch_obase;          // [nch+1] record offsets (words), first local obs
    int *ch_cam;                      // [2 nch] lowest / highest camera of a chunk's obs
    unsigned char *obs_lpt;           // [N] chunk-local point of each observation
    int max_blob;                     // term groups: largest chunk record
    int ngrp_mf;                      // leading MFMA groups
    // V*^-1 inside the MFMA Schur launch: each group's workgroup inverts the
    // damped V of its own points in its prologue, so no k_point_vinv launch.
    // Needs the MFMA groups' point ranges to tile every point [0, n) (checked
    // once at setup: no per-term groups, no long tracks; points no camera sees
    // lie inside the ranges and get their zero block).  VLGBA_VINV_FOLD=0
    // keeps the launch (A/B, tests).
    int vinv_fold;
    // long tracks (points [p_long, n), ba_plan.cpp build_plan): segment
    // chunks [nch_reg, nch), their V / eB partials, Schur tiles, update sums
    int nch_reg, nl, p_long;
    int *seg_pt, *seg_long;           // [nch - nch_reg] point, long index
    int *long_pt, *long_o0, *long_seg0;   // [nl], [nl+1] obs range, [nl+1] segments
    int *long_ebase;                  // [nl] first group e-slot
    // per camera its long-track observations in track order (k_schur_reduce
    // merges the lists of a block's two cameras): [m + 1], [nlobs], [nlobs]
    int *cam_lptr, *cam_lobs, *cam_ltrk;
    int max_lcam;                     // longest such list
    int long_o0_h;                    // first long-track observation (host copy)
    double *ylong;                    // [nlobs][3 NA] Y_a = W_a V*^-1 of each long observation
    // per block its long-track terms as (long obs of camera j, of camera k) pairs in
    // track order, found once at setup (k_long_pairs): [nb + 1], [pairs]
    int *lpair_ptr;
    int2 *lpair;
    int *lblk;     // blocks with long-track pairs, most pairs first (k_schur_long_acc)
    int nlb;       // their count (0: k_schur_reduce streams the pairs itself)
    double *vseg;                     // [nseg][12] V | eB partials per segment
    double *dpg_long;                 // [nl] point part of dp'(lambda dp + g)
    int mf_max_s, mf_max_e, mf_max_blob;   // MFMA groups' LDS sizes
    int *grp_ch, *grp_gs, *grp_ge;    // [ngrp+1] chunk / group-slot / group-eslot ranges
    unsigned short *cs_g, *ce_g;      // chunk slot / chunk e-slot -> group-local id
    int *blk_gptr, *blk_gslots;       // per block: its group slots in group order
    int *cam_gptr, *cam_gslots;       // per camera: its group e-slots in group order
    // optional outputs / inputs of the MEX-compatible stage entries (else NULL)
    double *xh_out;    // [N][2] projections (stage 1 and stage 3)
    double *B_out;     // [N][6] point Jacobians (stage 1)
    unsigned char *obs_vis;  // [N] stage 3: 0 = structural-only pair (no projection)
    int schur_owner;   // this rank adds U* / eA into the reduced system (every rank
                       // adds its own partials)
    int dpg_lambda;    // this rank adds the lambda dp'dp part of the camera dpg
    struct ba_ktimer *kt;   // NULL unless kernel timing is enabled
    hipStream_t stream;   // the library stream: never reassigned after setup
    // second stream of untimed single-rank passes, forked and joined with the
    // event pair: a plan without MFMA groups runs the camera reduction there,
    // beside V*^-1 and the Schur chunks (lm_pass), a mixed plan its per-term
    // groups beside the MFMA groups (ba_launch_schur_fast); k_schur_reduce,
    // the first consumer of either, waits for ev_join.  The launchers that can
    // run there take the stream as an argument.
    hipStream_t side;
    hipEvent_t ev_fork, ev_join;
    // host-mapped pass results: [0..5] the scal slots, [7] the pass sequence
    // number written last (k_publish, or the update's final sums when
    // ba_launch_update is asked to publish); the host spins on it instead of a
    // device-to-host copy + stream synchronisation
    volatile double *hres;     // host view
    double *hres_dev;          // device view
    unsigned long long seq;    // sequence number of the last publish launched
    unsigned *pub_cnt;         // device counter of k_sum_parts3's blocks (zeroed)
};

#define KT_B(d) \
    do { if ((d)->kt && (d)->kt->on) kt_begin((d)->kt, (d)->stream); } while (0)
#define KT_E(d, id) \
    do { if ((d)->kt && (d)->kt->on) kt_end((d)->kt, (d)->stream, (id)); } while (0)

#define BA_PART_MAX 65536

// CALL with NA a compile-time constant, for the camera models' sizes
#define BA_DISPATCH(NAEXPR, CALL)                                                   \
    switch (NAEXPR) {                                                               \
    case 6: { constexpr int NA = 6; CALL; } break;                                  \
    case 7: { constexpr int NA = 7; CALL; } break;                                  \
    case BA_RAD_NA: { constexpr int NA = BA_RAD_NA; CALL; } break;                  \
    case 10: { constexpr int NA = 10; CALL; } break;                                \
    case BA_PROJ_NA: { constexpr int NA = BA_PROJ_NA; CALL; } break;                \
    default: return -1000;                                                          \
    }

// ---- ba_kernels.hip ----
int ba_launch_rotations(ba_dev *d, const double *a, double *rot);
int ba_launch_linearize(ba_dev *d, ba_flags f);
// the fast path's camera reduction of the current linearisation (host only,
// launches nothing)
ba_camred ba_camred_args(const ba_dev *d, ba_flags f);
// U / eA (fast path: and the old SSE) now, on stream s: the library stream, or
// d->side in an untimed pass
int ba_launch_camera_reduce(ba_dev *d, ba_flags f, hipStream_t s);
int ba_launch_damp_point(ba_dev *d, double lambda);
int ba_launch_schur(ba_dev *d, double lambda);
int ba_launch_assemble(ba_dev *d);
// cam_updated: the solve directly before formed a_new / rot_new itself
// (ba_chol_solve), so no k_camera_update; false after every other writer of da.
// publish: the final-sums launch (k_sum_parts3: the fused and chunked updates)
// should also publish the pass's scalars to hres; *published (may be null)
// says whether a launch did, else the caller's ba_launch_publish has to
int ba_launch_update(ba_dev *d, double lambda, ba_flags f, bool cam_updated, bool publish,
                     bool *published);
int ba_launch_yeb(ba_dev *d);
// per observation (internal order) at the current parameters: e [N][2] = x - x_hat
// (unweighted), w [N], rho [N] of the context's loss; any pointer may be NULL
int ba_launch_obs_residuals(ba_dev *d, double *e, double *w, double *rho);
int ba_launch_publish(ba_dev *d);   // scal[0..5] + ++seq -> hres (host-mapped)
void *ba_dmalloc(size_t bytes);   // per-device caching allocator (ba_runtime.cpp)
// raise kernel fn's dynamic-LDS limit to >= bytes on the current device (cached
// per (kernel, device), thread-safe; ba_runtime.cpp)
int ba_ensure_dyn_lds(const void *fn, size_t bytes);
void ba_dfree(void *p);
// Typed device memory on that allocator and the asynchronous copies on a
// stream: 0 or -(int)hipError, as VLGBA_CHECK.  A count of 0 allocates one
// element and copies nothing.
template <typename T>
inline int dalloc(T **p, size_t count)
{
    *p = (T *)ba_dmalloc(sizeof(T) * (count ? count : 1));
    return *p ? 0 : -(int)hipErrorOutOfMemory;
}
template <typename T>
inline int upload(T *dst, const T *src, size_t count, hipStream_t s)
{
    if (count == 0) return 0;
    return -(int)hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, s);
}
template <typename T>
inline int download(T *dst, const T *src, size_t count, hipStream_t s)
{
    if (count == 0) return 0;
    return -(int)hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, s);
}
// move-only owner of one such block (freed with it; alloc() again replaces it).
// Work queued on a stream must have drained before the owner goes.
template <typename T>
class ba_dbuf {
    T *p_ = nullptr;

public:
    ba_dbuf() = default;
    ba_dbuf(ba_dbuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    ba_dbuf &operator=(ba_dbuf &&o) noexcept
    {
        if (this != &o) {
            ba_dfree(p_);
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ba_dbuf(const ba_dbuf &) = delete;
    ba_dbuf &operator=(const ba_dbuf &) = delete;
    ~ba_dbuf() { ba_dfree(p_); }
    int alloc(size_t count)
    {
        ba_dfree(p_);
        return dalloc(&p_, count);
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};
// after a re-solve: did one of the runner's own hand-offs time out?  Then the
// runner is off for this context (1); 0: no; < 0: error (ba_chol.hip)
int ba_env_runner_timed_out(ba_dev *d);
// fused damp + Vinv + Y + S + e_.  fold (or null): this pass's camera reduction,
// run by m + 1 workgroups appended to the MFMA Schur launch (needs ngrp_mf >
// 0).  side_camred: the side stream carries this pass's camera reduction, its
// end recorded in ev_join, so k_schur_reduce waits for it
int ba_launch_schur_fast(ba_dev *d, double lambda, const ba_camred *fold, bool side_camred);
// long tracks: count (fill = 0, into cnt[nb]) / write (fill = 1, at lpair_ptr) the
// per-block (obs, obs) pairs of k_schur_reduce (context setup)
int ba_launch_long_pairs(ba_dev *d, int fill, int *cnt);
int ba_launch_assemble_plain(ba_dev *d, double *S, long long ld, int lower_only);
// parity mode (ordered = 2): sequential LM scalars in the reference's flat order
int ba_launch_parity_old_sse(ba_dev *d);
int ba_launch_parity_new_sums(ba_dev *d, double lambda);
// ---- ba_chol.hip ----
// Everything below but ba_chol_free, ba_fix_diag_plain, ba_pinv_apply and
// ba_cr32_selinv_sources needs a solving context: d->chol set by ba_chol_setup
// (it is null in stage-mode contexts and after ba_chol_free).
int ba_chol_setup(ba_dev *d, const int *blk_jk_host, int nb);
void ba_chol_free(ba_dev *d);
int ba_chol_prepare(ba_dev *d);
int ba_assemble_tiles(ba_dev *d);   // envelope tiles of S + pinv rule + status, one launch
int ba_fix_diag_plain(ba_dev *d, double *S, long long ld);
int ba_chol_fix_diag(ba_dev *d);
// nospin = 1: only launches that never wait on other workgroups (the
// per-level / per-column paths) -- the re-solve after a hand-off timeout.
// *cam_updated = true when the solve also formed a_new / rot_new (the one-launch
// CR with camupd_fold), else false
int ba_chol_solve(ba_dev *d, bool *cam_updated, int nospin = 0);
// camera-aligned CR (cr32) only: the factor launches of the per-level path
// alone (no back substitution, da untouched); the selected
// inverse's tile sources on the host (src [2 * nt32]: tile holding Sigma_qp or
// -1, 1 when it is p's) and its descent on the device (src uploaded, sig
// [3][nt32][32 * 32]: Sigma_ee | Sigma_ep | Sigma_eq, row major)
int ba_cr32_factor(ba_dev *d);
int ba_cr32_selinv_sources(const ba_dev *d, int *src);
int ba_cr32_selinv(ba_dev *d, const int *src, double *sig);
// da = pinv(S) rhs from the eigen-decomposition S = V diag(ev) V^T (ev
// ascending, V column major ld x ld): MATLAB's tolerance ld * eps(max |ev|)
int ba_pinv_apply(ba_dev *d, const double *V, const double *ev, long long ld, const double *rhs,
                  double *work, double *da);

// ---- ba_pcg.hip (dense_solve = 5) ----
// the block CSR over both triangles, the work vectors, M^-1 (d->pcg; d->da
// must be allocated)
int ba_pcg_setup(ba_dev *d, const int *blk_jk_host, int nb);
void ba_pcg_free(ba_dev *d);
// da = the PCG iterate for sblk / rhs as the Schur phase left them (rhs gets
// its zeros on the exactly-zero rows); the status words scal[4] (failure) and
// scal[5] (0); d->pcg's statistics.  Synchronises the stream once per batch
int ba_pcg_solve(ba_dev *d);

// ---- ba_cov.hip (vlgba_covariance) ----
// track-length bins of k_point_cov: up to BA_COV_T8 views 8 lanes per point,
// up to BA_COV_T64 one wave, longer one workgroup; a long track's W rows are
// staged in LDS while they fit BA_COV_LDS bytes
#define BA_COV_T8 8
#define BA_COV_T64 32
#define BA_COV_LDS 65536
// fixed[r] = 1 for the exactly-zero rows of the dense lower S (before
// ba_fix_diag_plain gives them a unit diagonal)
int ba_cov_mark_fixed(ba_dev *d, const double *S, long long ld, unsigned char *fixed);
// the lower-triangle inverse -> full symmetric with the fixed rows / columns
// zeroed, and its diagonal blocks (na x na x m)
int ba_cov_finish(ba_dev *d, double *S, long long ld, const unsigned char *fixed, double *blocks);
// where k_point_cov reads Sigma_a[j,k] (k <= j): the finished dense inverse
// (packed == NULL), or a packed copy of its co-visible blocks -- block p of
// camera row j at rowptr[j] <= p < rowptr[j + 1] has column camera col[p]
// (ascending within a row), NA x NA doubles column major
struct ba_cov_src {
    const double *Sa;
    long long ld;
    const int *rowptr, *col;
    const double *packed;
};
// packed[p] = block (bj[p], bk[p]) of the dense S, p < nb
int ba_cov_pack(ba_dev *d, const double *S, long long ld, const int *bj, const int *bk, int nb,
                double *packed);
// the selected method: fixed[r] = 1 where the diagonal entry of row r in the
// co-visible blocks sblk is exactly zero or no diagonal block covers it (the
// rows ba_cov_mark_fixed finds in the dense S0 assembled from the same blocks)
int ba_cov_mark_fixed_blocks(ba_dev *d, unsigned char *fixed);
// ... and diag (na x na x m) and packed (block p = (bj[p], bk[p]), p < nb) from
// the selected inverse's tiles sig (ba_cr32_selinv), fixed rows / columns zero
int ba_cov_extract(ba_dev *d, const double *sig, const unsigned char *fixed, const int *bj,
                   const int *bk, int nb, double *diag, double *packed);
// Sigma_b of the points list[0 .. n8 + n64 + nwg) (internal order, binned by
// track length as above; tmax: the longest track) into out [n][9]; reads d->W
// and d->Vinv (lambda = 0)
int ba_launch_point_cov(ba_dev *d, const int *list, int n8, int n64, int nwg, int tmax,
                        const ba_cov_src *src, double *out);

#define TRY_RC(x)                                                                   \
    do {                                                                            \
        int rc__ = (x);                                                             \
        if (rc__) return rc__;                                                      \
    } while (0)
