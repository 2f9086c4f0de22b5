/*
 * vlgba.h -- C ABI of libvlgba, the MI355X (gfx950) bundle adjuster.
 *
 * Drop-in for the Levenberg-Marquardt paths of caomw/BundleAdjustmentMatlab
 * (VLG toolbox/bundle): Euclidean (bundle_euclid.m + mex_bundle_{1,2,3}) and
 * projective (bundle_projective.m + mex_bundle_proj_{1,2,3}).  Plain C:
 * pointers and sizes only, no C++ / torch / HIP types.  All arrays are fp64 column major in the reference's MATLAB
 * layouts unless stated otherwise; indices are 0-based int32.
 *
 * Return codes: 0 on success; VLGBA_E_* (< 0) for argument errors; a
 * negative hipError_t (-1 .. -999) for device failures.
 *
 * Threading: a vlgba_ctx is single-threaded (one HIP stream per context);
 * distinct contexts may be used from distinct threads.
 */
#ifndef VLGBA_H
#define VLGBA_H

#ifdef __cplusplus
extern "C" {
#endif

#define VLGBA_E_ARG (-1001)      /* bad size / option                        */
#define VLGBA_E_NUMA (-1002)     /* num_a not in {6, 7, 9, 10} (Euclidean) / 12 (projective);
                                    num_a = 9 where the radial model is not covered */
#define VLGBA_E_ORDER (-1003)    /* observation list not point-major / dups  */
#define VLGBA_E_NOMEM (-1004)    /* host allocation failed                    */
#define VLGBA_E_COMM (-1005)     /* RCCL failure                              */
#define VLGBA_E_ABI (-1006)      /* caller built against another vlgba.h      */
#define VLGBA_E_SINGULAR (-1007) /* vlgba_covariance: the undamped reduced camera
                                    system is not positive definite (gauge)   */

/* ABI of this header.  Bumped whenever a public struct, constant or entry
 * point changes: 1 = the round-1/2 layouts; 2 = vlgba_stats.pinv_passes /
 * spin_retries, vlgba_step_info.spin_retry, VLGBA_NPLAN 28; 3 =
 * vlgba_stats.nd_retries, vlgba_step_info.nd_retry, vlgba_comm_release,
 * VLGBA_NKERNELS 18 (k_update_linearize), vlgba_kernel_flops; 4 =
 * vlgba_debug_dehom; 5 = vlgba_debug_dehom removed, VLGBA_NPLAN 29 (the
 * envelope runner's launch count), vlgba_debug_force_status word 6; 6 =
 * vlgba_covariance, VLGBA_E_SINGULAR; 6 also covers the robust-loss entry
 * points added since (vlgba_set_loss, vlgba_get_loss, vlgba_get_residuals,
 * VLGBA_LOSS_*: entry points only, no struct changed) and the Jacobian-mode
 * ones (vlgba_set_jacobian, vlgba_get_jacobian, VLGBA_JAC_*: likewise) and the
 * covariance-method ones (vlgba_set_covariance_method,
 * vlgba_get_covariance_method, vlgba_get_covariance_blocks,
 * vlgba_debug_selinv_plan, VLGBA_COV_*: likewise), and the radial-distortion
 * camera num_a = 9 (a value vlgba_create refused before: no struct, constant or
 * entry point changed) and the batched per-point entries (vlgba_triangulate,
 * vlgba_intersect: entry points only) and their counterparts with a model, a
 * Jacobian mode and a loss (vlgba_resect_ex, vlgba_intersect_ex,
 * vlgba_triangulate_ex: likewise) and the block-Jacobi PCG reduced solve
 * (dense_solve = 5, a value vlgba_create refused before; vlgba_set_pcg,
 * vlgba_get_pcg, vlgba_get_pcg_stats, vlgba_debug_pcg_plan: entry points only;
 * VLGBA_NPLAN 33).  Callers
 * check it once at load time with VLGBA_ABI_CHECK() (the MEX gateways and the Python
 * loader do): the library compares the version and the struct sizes the
 * caller was compiled with against its own and returns 0 or VLGBA_E_ABI. */
#define VLGBA_ABI_VERSION 6

/* camera models (vlgba_problem.model) */
#define VLGBA_MODEL_EUCLIDEAN 0   /* bundle_euclid.m: a = [w; T; (K)], num_a 6/7/10;
                                     num_a = 9: radial distortion (below) */
#define VLGBA_MODEL_PROJECTIVE 1  /* bundle_projective.m: a = P(:) (3x4), num_a = 12   */

/* ------------------------------------------------------------------------
 * Problem: the reference's packed parameters and a COO observation list.
 *   a      num_a x m   [w; T; (K)] per camera  (bundle_euclid.m:88-96), or
 *                      P(:) per camera          (bundle_projective.m:70-73)
 *   b      3 x n       Xe(1:3,:)               (bundle_euclid.m:99;
 *                      Xp(1:3,:), bundle_projective.m:76)
 *   obs    visible (point, camera) pairs of x(1:2,:,:) / 'visibility'
 *          (bundle_euclid.m:50,71,102); any order, duplicates rejected.
 *
 * Radial distortion (Euclidean model, num_a = 9; beyond the reference): a =
 * [w(3); T(3); f; k1; k2] per camera -- one focal length and two radial
 * coefficients, the Bundler / BAL camera with a positive focal length and depth.
 * The principal point (cx, cy) = K[2], K[3] of the camera is fixed; K[0], K[1]
 * are unused (as for num_a = 7).  With Xc = R(w) b + T:
 *     u = Xc0 / Xc2, v = Xc1 / Xc2, r2 = u u + v v, d = 1 + k1 r2 + k2 r2 r2
 *     x = ( f (d u) + cx , f (d v) + cy )
 * Its Jacobians are closed form only (a forward difference with h = 1e-10 on k1
 * is noise): the context is created in VLGBA_JAC_ANALYTIC mode, whatever
 * VLGBA_JACOBIAN says, and vlgba_set_jacobian(ctx, VLGBA_JAC_FD) returns
 * VLGBA_E_ARG.  The back substitution uses all nine rows of da, whatever
 * vlgba_options.semantics says.  It runs on the fast path alone: vlgba_create
 * returns VLGBA_E_ARG for vlgba_options.ordered != 0 and for a problem that the
 * planner would hand to the ordered kernels (vlgba_plan_info [15]).  Robust
 * losses, covariances (both methods), the fix masks, every reduced solve and
 * sharded contexts work as for the other models; vlgba_resect_ex,
 * vlgba_intersect_ex and vlgba_triangulate_ex take the model too.  Not covered
 * (VLGBA_E_NUMA): vlgba_resect, the vlgba_mex_bundle_* stage entries, the MATLAB
 * drop-ins and the GPU scene generator.
 * ------------------------------------------------------------------------ */
typedef struct {
    int m;                 /* cameras                                            */
    int n;                 /* points                                             */
    int num_a;             /* 6 fix_calibration, 7 fix_principal, 10 variable K,
                              9 radial distortion (f, k1, k2); 12 projective    */
    long long num_obs;     /* visible observations                               */
    const int *obs_pt;     /* [num_obs] point index                              */
    const int *obs_cam;    /* [num_obs] camera index                             */
    const double *obs_x;   /* [2*num_obs] measured (u, v)                        */
    const double *K;       /* [4*m] fx fy cx cy (mex_bundle_1_XABeUVWeAeB.c:186);
                              unused (may be NULL) for the projective model      */
    double num_vis;        /* sum of the visibility values (bundle_euclid.m:82);
                              <= 0 means num_obs                                 */
    int model;             /* VLGBA_MODEL_*; 0 (zero-initialised) = Euclidean.
                              Projective: LM rule of bundle_projective.m:182-207
                              (errors / num_vis compared, lambda / 10 on accept,
                              * 10 on reject); fix_pivot is not an option there */
} vlgba_problem;

struct vlgba_step_info;

typedef struct {
    int fix_structure;           /* bundle_euclid.m:58-59                      */
    int fix_motion;              /* :60-61                                     */
    const unsigned char *pivot;  /* [m] or NULL: 'fix_pivot', pivot (:62-65)   */
    int verbose;                 /* 'verbose' (:73-74, printed to stdout)     */
    int max_iter;                /* 0 -> 20  (:117)                            */
    int max_iter2;               /* 0 -> 10  (:118)                            */
    double lambda0;              /* 0 -> 1e-3 (:111)                           */
    int device;                  /* HIP device ordinal                         */
    /* point sharding over ranks (one process per GPU); world_size <= 1: none  */
    int rank;
    int world_size;
    const void *comm_id;         /* 128-byte ncclUniqueId from rank 0, or NULL */
    /* reduced-camera solve (replaces pinv(S)*e_, bundle_euclid.m:193):
     * 0 (default) automatic -- block cyclic reduction (odd-even nested
     *   dissection, log2 depth) when S is tile-tridiagonal (co-visibility
     *   band narrower than 64 rows), else the envelope tile Cholesky;
     * 1: tile Cholesky over every lower tile (measurement);
     * 2: envelope tile Cholesky (tiles outside the envelope are exactly zero,
     *   so 1 and 2 give identical results);
     * 3: one-workgroup sequential Cholesky (parity mode, small problems);
 * 4: the envelope Cholesky on a nested-dissection camera order whenever the
 *   cameras split into independent arcs + a separator (0 takes that order
 *   when it shortens the chain of factor steps by a quarter or more).
     * 5: block-Jacobi preconditioned conjugate gradients on the co-visible
     *   blocks themselves (opt-in; no dense S is allocated: device memory
     *   linear in the blocks and cameras).  An inexact step: the iteration
     *   stops at sqrt(r'M^-1 r / e_'M^-1 e_) <= tol or at the iteration limit
     *   (vlgba_set_pcg), and the iterate is the step either way.  Fast path
     *   only: VLGBA_E_ARG with ordered != 0 and on a problem the planner
     *   hands to the ordered kernels.
     * Any of them meeting a non-positive pivot (5: in a camera's diagonal
     * block, or p'Sp <= 0, or a scalar that is not finite) falls back to
     * pinv(S) e_ from a symmetric eigen-decomposition on the GPU
     * (vlgba_step_info.pinv)                                                 */
    int dense_solve;
    /* 1: "ordered" mode -- every sum over points runs sequentially in
     * ascending point order exactly as the reference loops do, making the
     * reduced system bit-identical to the reference arithmetic; 2: "parity"
     * mode -- ordered, plus the sequential Cholesky (dense_solve 3) and the LM
     * scalars e'e, dp'(lambda dp + g) summed in the reference's flat order,
     * so the whole LM trajectory (error_, a, b) is bit-identical to the CPU
     * oracle's (single rank, small problems); 0 (default): the fused chunked
     * Schur path (same terms, sums grouped per chunk of points, deterministic
     * run to run)                                                            */
    int ordered;
    /* world_size > 1 without comm_id: a host collective instead of RCCL.  The
     * library copies the buffer to host memory, calls allreduce(buf, count,
     * user), which must leave the element-wise sum over ranks in buf and
     * return 0, and copies it back (e.g. gloo via torch.distributed). */
    int (*allreduce)(double *buf, long long count, void *user);
    void *allreduce_user;
    /* fast-path Schur complement kernel (ordered = 0): 0 (default) automatic --
     * dense per-chunk Y W^T products on fp64 MFMA when every point has at most
     * 16 * (num_a == 6 ? 3 : 4) / num_a observations, else per-term sums;
     * 1: per-term sums (measurement / cross-check).  Same terms either way. */
    int schur_kernel;
    /* driver semantics: 0 (default) bundle_euclid.m (MEX-backed: the back
     * substitution uses da(1:6,j) only, mex_bundle_3_db_new.c:113-120, App. A
     * Q3; 'fix_pivot' honoured); 1 bundle_euclid_nomex.m (the pure-MATLAB
     * twin: db uses all num_a rows of da, bundle_euclid_nomex.m:268-277; no
     * fix_pivot -- pivot is ignored) */
    int semantics;
    /* stop rule of bundle_euclid.m:123: stop once the accepted step lowers
     * error_ by no more than stop_rel * error_(previous); 0 -> 1e-3          */
    double stop_rel;
    /* per-pass log hook (NULL: none): vlgba_run calls on_pass(pass, iter, info,
     * user) after every LM pass (1-based pass counter, iter = the reference's
     * iteration counter after the pass, bundle_euclid.m:221), on the calling
     * thread, rank 0 only; bundle.py writes it as one JSON line per pass */
    void (*on_pass)(int pass, int iter, const struct vlgba_step_info *info, void *user);
    void *on_pass_user;
} vlgba_options;

typedef struct {
    int iterations;        /* LM passes (accepted + rejected)                 */
    int accepted;          /* accepted steps                                  */
    int num_error;         /* entries written to error_out                    */
    double lambda;         /* final damping                                   */
    double seconds;        /* wall time of the solve (setup excluded)         */
    int pinv_passes;       /* passes whose step came from the pinv fallback   */
    int spin_retries;      /* passes re-solved after a hand-off spin timeout  */
    int nd_retries;        /* passes whose nested-dissection Cholesky met a
                              non-positive pivot and the natural-order Cholesky
                              (rocSOLVER dpotrf) took the step instead        */
} vlgba_stats;

/* One LM pass, for benchmarking / custom drivers. */
typedef struct vlgba_step_info {
    double old_sse;        /* e'e before the step (bundle_euclid.m:209)       */
    double new_sse;        /* e_new'e_new (:210)                              */
    double dpg;            /* dp'(lambda dp + g) (:217)                       */
    double rho;
    double lambda;         /* lambda used by this pass                        */
    int accepted;
    int chol_failed;       /* non-positive pivot in the reduced solve: the
                              step came from the pinv fallback (= pinv)       */
    int pinv;              /* da = pinv(S) e_ by eigen-decomposition: a dense
                              (num_a m)^2 copy of S + rocSOLVER dsyevd, i.e.
                              8 (num_a m)^2 bytes of device memory and
                              O((num_a m)^3) flops (cfg3: 288 MB); the library
                              notes each such pass on stderr (ld, seconds)    */
    int spin_retry;        /* the one-launch solve gave up waiting on a
                              hand-off (a bounded spin): the pass was solved
                              again with the per-level launches (every rank
                              takes the same decision: the status words are
                              all-reduced with the pass scalars)              */
    int nd_retry;          /* the nested-dissection order met a non-positive
                              pivot; the natural-order dpotrf solved the pass
                              (pinv = 0) or failed too (pinv = 1)             */
} vlgba_step_info;

typedef struct vlgba_ctx vlgba_ctx;

/* ---- fused solver: the whole bundle_euclid.m LM loop on the GPU -----------
 * Replaces bundle_euclid.m:111-249 (and its three MEX calls :139,192,204).
 * a (num_a*m) and b (3*n) are read as the start point and overwritten with
 * the result.  error_out (may be NULL) receives error_ (SSE / num_vis per
 * accepted step, :219-231): at most error_cap entries are written (error_ has
 * at most max_iter entries; stats->num_error is its full length). */
int vlgba_solve(const vlgba_problem *prob, const vlgba_options *opt, double *a, double *b,
                double *error_out, int error_cap, vlgba_stats *stats);

/* ---- handle API -------------------------------------------------------- */
int vlgba_create(const vlgba_problem *prob, const vlgba_options *opt, vlgba_ctx **out);
int vlgba_set_params(vlgba_ctx *ctx, const double *a, const double *b);
int vlgba_get_params(vlgba_ctx *ctx, double *a, double *b);
/* one LM pass at the context's lambda; relinearize != 0 forces stage 1 even
 * when the previous pass was rejected (bench: every pass does full work).
 * update_lm != 0 applies the accept/reject rule (:218-241) to the context. */
int vlgba_step(vlgba_ctx *ctx, int relinearize, int update_lm, vlgba_step_info *info);
/* stage 1 at the current parameters (mex_bundle_1_XABeUVWeAeB.c outputs, the
 * reduced forms of bundle_euclid.m:139-154) -- the one the context holds when
 * it is current (after a rejected step, or the fast path's fused update after
 * an accepted one), else computed: U (num_a x num_a x m), eA
 * (num_a x m) summed over all ranks; V (3 x 3 x n_local), eB (3 x n_local) and
 * W (num_a x 3 per observation, observations point-major: points ascending,
 * cameras ascending within a point) for this rank's points.  Any pointer may
 * be NULL.  Also marks the linearisation valid for the next vlgba_step.
 * With a loss set (vlgba_set_loss) these are the weighted quantities: every
 * observation's Jacobian rows and residual times sqrt(w).
 * In analytic-Jacobian mode (vlgba_set_jacobian) A and B are the closed-form
 * derivatives: U, V, W, eA, eB are exact to fp64 rounding instead of the
 * forward differences' ~1e-6; the residuals in eA, eB are the same bits. */
int vlgba_get_linearization(vlgba_ctx *ctx, double *U, double *eA, double *V, double *eB,
                            double *W);
/* the LM loop from the context's parameters; error_out / error_cap as
 * vlgba_solve.  Every handle entry point makes the context's device current.
 * The accept / lambda / stop decisions are the host's (a handful of scalars
 * per pass, as bundle_euclid.m keeps them in MATLAB). */
int vlgba_run(vlgba_ctx *ctx, double *error_out, int error_cap, vlgba_stats *stats);
/* npass full passes at the context's parameters and lambda, each
 * relinearising, none changing the context (vlgba_step(ctx, 1, 0, .) npass
 * times); info: the last pass */
int vlgba_run_passes(vlgba_ctx *ctx, int npass, vlgba_step_info *info);
/* the last pass's step: da (num_a * m, the reduced solve) and db (3 x
 * n_local, this rank's points); either may be NULL */
int vlgba_get_step(vlgba_ctx *ctx, double *da, double *db);
/* the reduced camera system at the context's lambda (mex_bundle_2_Se_ output,
 * bundle_euclid.m:192): the co-visible blocks S_jk, j >= k (num_a x num_a
 * column major each, lower triangle meaningful for j == k; count =
 * vlgba_plan_info [10]) with their camera pairs blk_jk [2 * count], and e_
 * (num_a * m).  Linearises first if the parameters changed.  NULL skips.
 * With a loss set: the reduced system of the weighted normal equations. */
int vlgba_get_reduced_system(vlgba_ctx *ctx, int *blk_jk, double *blocks, double *e_);
/* Posterior covariance at the context's parameters (linearises first if they
 * changed, as vlgba_get_reduced_system does), undamped (lambda = 0), with the
 * context's fix masks applied exactly as a pass applies them
 * (bundle_euclid.m:140-154):
 *   S0      = U - sum_i W_i V+_i W_i^T               reduced camera system
 *   Sigma_a = S0^-1                                   (num_a m)^2
 *   Sigma_b_i = V+_i + V+_i (sum_{j,k in cams(i)} W_ij^T Sigma_a[j,k] W_ik) V+_i
 *   sigma2  = SSE / dof,  dof = 2 num_obs - (free camera rows
 *             + 3 (points with an observation, or 0 under fix_structure))
 * V+_i is the 3x3 pseudo-inverse the passes use at lambda = 0 (the same code).
 *   cov_a       [num_a x num_a x m]  diagonal blocks of Sigma_a   (NULL: skip)
 *   cov_a_full  [ld x ld], ld = num_a*m, full symmetric Sigma_a   (NULL: skip)
 *   cov_b       [3 x 3 x n]          Sigma_b_i                    (NULL: skip)
 *   info        [8] or NULL: [0] SSE  [1] dof  [2] sigma2  [3] fixed rows
 *               [4] ms assemble + factor + inverse   [5] ms point kernel
 *               [6] device bytes of dense scratch    [7] 0
 * scale != 0 multiplies every output by sigma2 (VLGBA_E_ARG when dof <= 0;
 * info is written first).
 * Fixed parameters: a row of S0 that is exactly zero (a pivot camera, every
 * camera under fix_motion, a camera without observations, the rotation rows
 * of a camera with |w| < 1e-6) is factored with a unit diagonal, as the
 * passes do, and its row and column are exactly 0 in every output.  An unseen
 * point, and every point under fix_structure, has Sigma_b_i = 0 exactly.
 * Gauge: the covariance is conditional on what the caller fixed.  When the
 * Cholesky factorisation (rocSOLVER dpotrf, then dpotri) meets a non-positive
 * pivot the call returns VLGBA_E_SINGULAR and writes no covariance; no
 * pseudo-inverse (free-gauge) covariance is attempted.  The Jacobians are the
 * reference's forward differences (h = 1e-10): an unfixed gauge usually leaves
 * S0 ill-conditioned rather than exactly singular, the call then succeeds with
 * the large values that implies, and every value carries the Jacobians'
 * relative noise of about 1e-6.  In analytic-Jacobian mode
 * (vlgba_set_jacobian) they are the closed-form derivatives: that noise is
 * gone, and the rotation rows of a camera with |w| < 1e-6 are no longer zero,
 * so they are not fixed rows.
 * One rank only: VLGBA_E_ARG for world_size > 1 (with or without a
 * communicator); VLGBA_E_ARG too when rocSOLVER or its dpotrf / dpotri are not
 * available.  Uses 8 ld^2 bytes of device scratch (the pinv fallback's
 * buffer; cfg3: 288 MB).  The selected method (vlgba_set_covariance_method
 * below) avoids the dense ld^2 step on contexts whose reduced solve is the
 * camera-aligned cyclic reduction.
 * The call leaves the LM state as it was: the next vlgba_step gives the same
 * bits as without it, vlgba_get_step still returns the last pass's step.
 * With a loss set (vlgba_set_loss) the unscaled outputs come from the weighted
 * linearisation and info[0] is the robust cost sum rho(s); scale != 0 then
 * returns VLGBA_E_ARG: sigma2 from a robust cost is not the noise variance. */
int vlgba_covariance(vlgba_ctx *ctx, int scale, double *cov_a, double *cov_a_full,
                     double *cov_b, double *info);
/* ---- how vlgba_covariance forms Sigma_a --------------------------------------
 *   VLGBA_COV_DENSE     the dense inverse described above (default)
 *   VLGBA_COV_SELECTED  a selected inverse on the factors of the camera-aligned
 *                       cyclic reduction: Sigma_a only on the tile-tridiagonal
 *                       pattern of S0, which holds every co-visible block
 * The selected method assembles S0 in the reduced solve's own tiles, runs the
 * cyclic reduction's per-level factor launches (no back substitution: the last
 * pass's step stays), then walks the elimination tree back down, one launch
 * per level:  for a tile e eliminated between the kept tiles p < e < q, with
 * L_e = chol(D_e), Mp = L_e^-T L(p, e)^T, Mq = L_e^-T L(q, e)^T,
 *   Sigma_ep = -(Mp Sigma_pp + Mq Sigma_qp)
 *   Sigma_eq = -(Mp Sigma_qp^T + Mq Sigma_qq)
 *   Sigma_ee = L_e^-T L_e^-1 - Sigma_ep Mp^T - Sigma_eq Mq^T
 * cov_a and the co-visible blocks behind cov_b come out of those tiles; the
 * point stage is the dense method's kernel on the packed blocks (whatever
 * VLGBA_COV_PACKED says: that switch concerns the dense method).  Its device
 * scratch is three 32 x 32 tiles per cyclic-reduction tile (info[6]; cfg3:
 * 4.9 MB); neither rocSOLVER nor the 8 ld^2 buffer is touched.  info[4] is
 * then the time of Schur + assembly + factor + descent + extraction.  Fixed
 * rows, info[0..3], scaling, the loss and Jacobian semantics, the single-rank
 * rule and "the call leaves the LM state as it was" are the dense method's.  A
 * non-positive pivot of the cyclic reduction returns VLGBA_E_SINGULAR and
 * writes no covariance.  Summation order is fixed: a call repeated on the
 * same state gives the same bits; they differ from the dense method's by
 * rounding.
 * vlgba_set_covariance_method: VLGBA_E_ARG for an unknown kind, and for
 * VLGBA_COV_SELECTED unless the context's reduced solve is the camera-aligned
 * cyclic reduction (vlgba_plan_info [12] > 0 and [19] == num_a * floor(32 /
 * num_a)) on one rank, not in ordered or parity mode.  With
 * VLGBA_COV_SELECTED, vlgba_covariance returns VLGBA_E_ARG when cov_a_full !=
 * NULL: the full matrix is the dense method's.
 * Not built: selected inverses on the envelope, nested-dissection and 64-row
 * cyclic-reduction factors, several ranks, the MATLAB drop-ins. */
#define VLGBA_COV_DENSE 0
#define VLGBA_COV_SELECTED 1
int vlgba_set_covariance_method(vlgba_ctx *ctx, int kind);
int vlgba_get_covariance_method(vlgba_ctx *ctx, int *kind);
/* the co-visible blocks Sigma_a[j,k], j >= k, of the last successful
 * vlgba_covariance call (either method; scaled by sigma2 if that call was), in
 * the order and layout of vlgba_get_reduced_system: blk_jk [2 * count], blocks
 * [num_a x num_a x count] column major, count = vlgba_plan_info [10]; both
 * triangles of a diagonal block are filled.  Either pointer may be NULL.
 * VLGBA_E_ARG before any successful call. */
int vlgba_get_covariance_blocks(vlgba_ctx *ctx, int *blk_jk, double *blocks);
/* ---- robust loss (iteratively reweighted least squares, first order) -----
 * s = e0^2 + e1^2 of an observation in pixels^2, scale c in pixels, w = rho'(s):
 *   VLGBA_LOSS_NONE    rho = s                                     w = 1
 *   VLGBA_LOSS_HUBER   rho = s (s <= c^2), else 2 c sqrt(s) - c^2  w = 1, else c / sqrt(s)
 *   VLGBA_LOSS_CAUCHY  rho = c^2 log1p(s / c^2)                    w = 1 / (1 + s / c^2)
 * The observation's Jacobian rows and residual are multiplied by sqrt(w)
 * where they are formed, so U, V, W, eA, eB are the weighted normal equations
 * (Gauss-Newton on the robust cost, no second-order correction) and g the
 * robust gradient; the LM scalars are the robust cost: vlgba_step_info.old_sse
 * / new_sse hold sum rho(s), rho = (old - new) / dpg.  The accept rule, the
 * stop rule and error_ (cost / num_vis) keep their form.  Weights are local
 * to an observation: sharded contexts need no further collective, every rank
 * sets the same loss.
 * vlgba_set_loss: VLGBA_E_ARG for an unknown kind, for a non-finite or <= 0
 * scale when kind != VLGBA_LOSS_NONE, and for a context in ordered or parity
 * mode (vlgba_options.ordered != 0), whose purpose is bit parity with a
 * reference that has no loss.  Marks the linearisation stale: the next pass or
 * getter linearises again.  VLGBA_LOSS_NONE restores the plain solver exactly.
 * Not covered (they stay plain least squares): vlgba_resect and vlgba_intersect
 * (vlgba_resect_ex and vlgba_intersect_ex take a loss), the vlgba_mex_bundle_*
 * stage entries and the MATLAB drop-ins, which keep the reference's option
 * list. */
#define VLGBA_LOSS_NONE 0
#define VLGBA_LOSS_HUBER 1
#define VLGBA_LOSS_CAUCHY 2
int vlgba_set_loss(vlgba_ctx *ctx, int kind, double scale);
int vlgba_get_loss(vlgba_ctx *ctx, int *kind, double *scale);
/* ---- Jacobians of the fused LM path -----------------------------------------
 *   VLGBA_JAC_FD        the reference's forward differences, h = 1e-10 (default)
 *   VLGBA_JAC_ANALYTIC  closed-form derivatives of the same projection
 * The analytic mode changes only the Jacobian columns A, B of the fast path's
 * linearisation: x_hat, the residuals, the SSE (vlgba_step_info.old_sse /
 * new_sse at equal parameters) and vlgba_get_residuals are bit for bit those of
 * VLGBA_JAC_FD.  The derivative of the rotation is that of the exponential
 * map; for |w| < 1e-6, where the projection uses R = I exactly (vl_rodrigues),
 * it is the limit [e_k]x -- so a camera that starts at w = 0 rotates, which
 * under forward differences it never does (its rotation columns are exactly
 * zero).  Composes with vlgba_set_loss and sharded contexts (every rank sets
 * the same mode).
 * vlgba_set_jacobian: VLGBA_E_ARG for an unknown kind and for a context that
 * runs the ordered kernels: ordered or parity mode (vlgba_options.ordered != 0),
 * and a problem that the planner hands to them although ordered == 0 was asked
 * for (a track of more than 65535 views, long tracks of more than 2^26 terms
 * in all; vlgba_plan_info [15] tells).  Rebuilds the rotation table of the
 * current parameters and marks the linearisation stale.  VLGBA_JAC_FD restores
 * the default solver exactly.  The environment variable VLGBA_JACOBIAN=analytic
 * makes analytic the default of every context created with ordered == 0 that
 * stays on the fast path; one the planner hands to the ordered kernels stays
 * VLGBA_JAC_FD (vlgba_get_jacobian tells).  The radial-distortion camera
 * (num_a = 9) has the analytic mode only: VLGBA_JAC_FD is VLGBA_E_ARG there, and
 * the environment variable has no effect on it.  Not covered (forward differences always): ordered /
 * parity mode, vlgba_resect and vlgba_intersect (vlgba_resect_ex and
 * vlgba_intersect_ex take the mode), the vlgba_mex_bundle_* stage entries and
 * the MATLAB drop-ins. */
#define VLGBA_JAC_FD 0
#define VLGBA_JAC_ANALYTIC 1
int vlgba_set_jacobian(vlgba_ctx *ctx, int kind);
int vlgba_get_jacobian(vlgba_ctx *ctx, int *kind);
/* ---- the block-Jacobi PCG reduced solve (vlgba_options.dense_solve = 5) ----
 * Preconditioned conjugate gradients on S da = e_ from da = 0, M_j the diagonal
 * block of camera j; after iteration k the solve stops when sqrt(rz_k / rz_0)
 * <= tol (rz = r'M^-1 r) or k == max_iter, and the iterate is the step (every
 * CG iterate from zero is a descent direction of the damped model).  A row
 * whose diagonal entry is exactly 0 (a pivot camera, fix_motion, a camera
 * without observations) gets a unit diagonal and a zero right-hand side: da is
 * exactly 0 there.  Deterministic: two calls on the same state give the same
 * bits and the same iteration count, on every rank of a sharded context.
 * tol <= 0 or max_iter <= 0 keeps the current value; VLGBA_E_ARG for a non-finite tol,
 * tol >= 1, and a context whose solver is not the PCG.  Defaults: tol 0.1, max_iter 500. */
int vlgba_set_pcg(vlgba_ctx *ctx, double tol, int max_iter);
int vlgba_get_pcg(vlgba_ctx *ctx, double *tol, int *max_iter);
/* the last pass's solve: iterations run, sqrt(rz_k / rz_0) at its end, 1 when the tolerance
 * was met; total: iterations summed over the context's passes (any pointer may be NULL) */
int vlgba_get_pcg_stats(vlgba_ctx *ctx, int *iterations, double *relres, int *converged,
                        long long *total);
/* per observation of this rank at the context's current parameters, in the
 * order of vlgba_get_linearization's W rows (point-major, cameras ascending
 * within a point): e [2 x N_local] the unweighted residuals x - x_hat, w
 * [N_local] the loss's weights and rho [N_local] its costs (no loss: w = 1,
 * rho = s).  Any pointer may be NULL.  Computed on demand (the passes store
 * nothing per observation); leaves the LM state untouched. */
int vlgba_get_residuals(vlgba_ctx *ctx, double *e, double *w, double *rho);
int vlgba_sync(vlgba_ctx *ctx);
void vlgba_destroy(vlgba_ctx *ctx);
/* device-kernel timing of the last vlgba_step, milliseconds per phase:
 * [0] linearize [1] camera reduce [2] damp/Y [3] schur [4] assemble
 * [5] cholesky+solve [6] update; requires vlgba_set_timing(ctx, 1) first. */
int vlgba_set_timing(vlgba_ctx *ctx, int on);
int vlgba_phase_ms(vlgba_ctx *ctx, double *ms7);
/* per-kernel device time accumulated over the passes run with timing on
 * (HIP events around every launch): ms[k], calls[k] for k < VLGBA_NKERNELS,
 * named by vlgba_kernel_name(k); reset = 1 clears the accumulators.  ctx NULL:
 * the process-wide sums of the contexts destroyed with timing on (environment
 * VLGBA_KTIME_ALL=1 switches timing on at every vlgba_create: the growing
 * replay's device-busy time). */
#define VLGBA_NKERNELS 18
int vlgba_kernel_ms(vlgba_ctx *ctx, double *ms, long long *calls, int reset);
/* the reduced solve's algorithmic flops (vlgba_plan_info [25..27]) of the timed
 * passes, on the timer that ran them (k_cr_factor / k_factor_step, k_syrk,
 * k_cr_back / k_backward); ctx NULL: process-wide as vlgba_kernel_ms.  Cleared
 * by vlgba_kernel_ms(.., reset = 1). */
int vlgba_kernel_flops(vlgba_ctx *ctx, double *flops);
const char *vlgba_kernel_name(int k);
/* execution-plan sizes of this rank (roofline accounting in bench.py):
 * [0] observations [1] points [2] cameras [3] num_a [4] Schur chunks
 * [5] chunk block slots [6] chunk camera slots [7] Schur groups [8] group
 * block slots [9] group camera slots [10] co-visible blocks (j >= k)
 * [11] 64-row tiles of S [12] cyclic-reduction levels (0: tile Cholesky)
 * [13] eliminated tiles [14] kept-tile updates [15] ordered mode
 * [16] Schur (obs, obs) terms [17] chunk metadata words [18] MFMA Schur
 * chunks in use [19] rows per cyclic-reduction tile (64, or NA * floor(32 /
 * NA) for the camera-aligned tiles; 0 without cyclic reduction) [20] MFMA
 * Schur groups (the leading ones; the rest use per-term sums) [21] points
 * reordered internally (1: short tracks first, input order restored at the
 * API) [22] long tracks (more views than a Schur chunk holds: segment chunks
 * + the long-track kernels) [23] nested-dissection arcs of the envelope
 * Cholesky (0: natural camera order) [24] its separator tiles [25] the
 * reduced solve's algorithmic flops in the launches timed as k_factor_step /
 * k_cr_factor (the one-launch cyclic reduction: all of it) [26] in the
 * separator SYRK (k_syrk) [27] in the backward solve (k_backward / k_cr_back):
 * tile-dense potrf + trtri, GEMMs and GEMVs, each counted once [28] envelope
 * runner launches (k_env_runner, opt-in VLGBA_ENV_RUNNER=1) made by this
 * context so far [29] 1: the MFMA Schur launch forms V*^-1 itself (no
 * k_point_vinv launch; VLGBA_VINV_FOLD=0 or a plan whose MFMA groups do not
 * tile every point: 0) [30] 1: the one-launch cyclic reduction does the camera
 * update (no k_camera_update launch after it; VLGBA_CAMUPD_FOLD=0 or another
 * solver: 0) [31] 1: the reduced solve is the block-Jacobi PCG (dense_solve =
 * 5; [11]-[14], [19] and [23]-[28] are then 0) [32] bytes of device memory the
 * reduced solve itself holds, without the blocks and e_ every solver has: for
 * the direct solvers the dense S, the tile inverses and the lists of the
 * chosen method (>= 8 lds^2, lds = NA * cameras rounded up to 64); for the
 * PCG, with ld = [3] * [2], m = [2], nb = [10],
 *   8 (4 + NA) ld + ld + 16 ceil(m / 4) + 64 + 8 m + 4 + 24 nb
 * (r, z, p, q; the M_j^-1 blocks; the zero-row mask; the dot products'
 * partial sums; the state words; the block CSR over both triangles with room
 * for 2 nb entries): no ld^2 term.  Writes min(len, VLGBA_NPLAN) entries, returns
 * VLGBA_NPLAN (a caller built for fewer entries keeps working: entries are
 * only ever appended, without an ABI bump). */
#define VLGBA_NPLAN 33
int vlgba_plan_info(vlgba_ctx *ctx, long long *info, int len);

/* ---- stage entries with the reference MEX argument layouts ---------------
 * Host pointers in, host pointers out; every output is fully written (zeros
 * / X for invisible pairs, as the MEX files leave them).  vis is n x m
 * (non-zero = visible, bundle_euclid.m:81). */

/* [X_hat A B e U V W eA eB] = mex_bundle_1_XABeUVWeAeB(K, a, b, X, visible)
 * replaces toolbox/bundle/mex_bundle_1_XABeUVWeAeB.c:72-337. */
int vlgba_mex_bundle_1(int m, int n, int num_a, const double *K, const double *a,
                       const double *b, const double *X, const double *vis,
                       double *X_hat, double *A, double *B, double *e, double *U, double *V,
                       double *W, double *eA, double *eB);

/* [S e_] = mex_bundle_2_Se_(Y, W, U, eA, eB)
 * replaces toolbox/bundle/mex_bundle_2_Se_.c:15-158.  The co-visibility
 * pattern is taken from the non-zero W_ij / Y_ij blocks (exact: the
 * reference adds exact zeros for the others). */
int vlgba_mex_bundle_2(int m, int n, int num_a, const double *Y, const double *W,
                       const double *U, const double *eA, const double *eB, double *S,
                       double *e_);

/* [db a_new b_new X_hat] = mex_bundle_3_db_new(W, da, eB, V_inv, K, a, b, X, visible)
 * replaces toolbox/bundle/mex_bundle_3_db_new.c:12-170 (db :99-134 uses da(1:6,j)
 * only, as the reference does). */
int vlgba_mex_bundle_3(int m, int n, int num_a, const double *W, const double *da,
                       const double *eB, const double *Vinv, const double *K, const double *a,
                       const double *b, const double *X, const double *vis, double *db,
                       double *a_new, double *b_new, double *X_hat);

/* Projective stages (mex_bundle_proj_*.c: the same layouts with num_a = 12
 * and no K):
 * [X_hat A B e U V W eA eB] = mex_bundle_proj_1_XABeUVWeAeB(a, b, X, visible)
 * replaces toolbox/bundle/mex_bundle_proj_1_XABeUVWeAeB.c:88-332. */
int vlgba_mex_bundle_proj_1(int m, int n, const double *a, const double *b, const double *X,
                            const double *vis, double *X_hat, double *A, double *B, double *e,
                            double *U, double *V, double *W, double *eA, double *eB);

/* [S e_] = mex_bundle_proj_2_Se_(Y, W, U, eA, eB)
 * replaces toolbox/bundle/mex_bundle_proj_2_Se_.c:15-158 (num_a = 12). */
int vlgba_mex_bundle_proj_2(int m, int n, const double *Y, const double *W, const double *U,
                            const double *eA, const double *eB, double *S, double *e_);

/* [db a_new b_new X_hat] = mex_bundle_proj_3_db_new(W, da, eB, V_inv, a, b, X, visible)
 * replaces toolbox/bundle/mex_bundle_proj_3_db_new.c:34-178 (db uses
 * da(1:6,j) only, :107-121, as the Euclidean stage does). */
int vlgba_mex_bundle_proj_3(int m, int n, const double *W, const double *da, const double *eB,
                            const double *Vinv, const double *a, const double *b,
                            const double *X, const double *vis, double *db, double *a_new,
                            double *b_new, double *X_hat);

/* ---- batched one-camera refinement with the structure fixed ---------------
 * The bundle_euclid call of estimate_camera.m:247-253,
 *   bundle_euclid(K, T, Omega, X, x0, ['fix_calibration',] 'fix_structure',
 *                 'visibility', inlier')
 * for nprob independent cameras at once (one workgroup per camera and LM
 * pass; the LM rule of bundle_euclid.m:111-241 per camera on the host).  Each
 * camera's trajectory equals the parity-mode solver's (and the CPU oracle's)
 * bit for bit.  Camera q sees observations obs_ptr[q] .. obs_ptr[q+1]-1 of
 * fixed points X (3 per observation) measured at x (2 per observation);
 * num_vis = its observation count. */
typedef struct {
    int nprob;
    int num_a;                 /* 6 fix_calibration, 7 fix_principal, 10 free K;
                                  vlgba_resect_ex alone: 9 radial distortion    */
    const long long *obs_ptr;  /* [nprob + 1], obs_ptr[0] = 0                  */
    const double *X;           /* [3 * N] world point of each observation      */
    const double *x;           /* [2 * N] measured (u, v)                       */
    const double *K;           /* [4 * nprob] fx fy cx cy                       */
} vlgba_resect_problem;

/* a (num_a x nprob, [w; T; (K)] per camera) is the start point and receives the
 * result; error_out (nprob x error_cap, row q = camera q's error_) and
 * num_error (nprob) may be NULL.  opt: max_iter, max_iter2, lambda0,
 * stop_rel, device are honoured (the rest does not apply).  stats (may be
 * NULL): iterations / accepted summed over the cameras, camera 0's lambda,
 * pinv_passes the camera passes whose num_a x num_a Cholesky met a pivot that
 * was not positive. */
int vlgba_resect(const vlgba_resect_problem *prob, const vlgba_options *opt, double *a,
                 double *error_out, int error_cap, int *num_error, vlgba_stats *stats);

/* ---- batched per-point entries: the dual of vlgba_resect -------------------
 * m pinhole Euclidean cameras K (4 x m: fx fy cx cy), T (3 x m), w (3 x m) and
 * n points given by their tracks in CSR form: point i has the views
 * obs_ptr[i] .. obs_ptr[i+1]-1 (obs_ptr[0] = 0), view o is seen by camera
 * obs_cam[o] (any order within a point) at obs_x[2 o], obs_x[2 o + 1].
 * VLGBA_E_ARG, before any device work, for a NULL pointer, m < 1, n < 0, a
 * non-monotone obs_ptr and a camera id outside [0, m); n == 0 succeeds without
 * a launch.  Host pointers in and out; thread-safe (a stream per call).
 * Not covered by these two entries: the radial model, robust losses, analytic
 * Jacobians (vlgba_intersect_ex and vlgba_triangulate_ex below take them); by
 * none: the projective model, several GPUs, the MATLAB drop-ins. */

/* X = triangulation(P, x) for every point (replaces toolbox/geometry/
 * triangulation.m:19-53): P_j = calibration_matrix(K_j) [R(w_j) T_j], the rows
 * u P_j(3,:) - P_j(1,:), v P_j(3,:) - P_j(2,:) of every view stacked into A, X
 * the right singular vector of A's smallest singular value over its 4th entry
 * (here: the eigenvector of A'A by cyclic Jacobi), X = (0, 0, 0, 0) when
 * P_j(3,:) X < 0 in any view.  One lane per point.  X (4 x n); status (n, may
 * be NULL): 1 triangulated, 0 rejected by the depth test, 2 fewer than two
 * views or a non-finite result (X zeros for 0 and 2).  A deliberate deviation:
 * the reference returns inf / nan when v(4) == 0 (a point at infinity); this
 * entry returns zeros with status 2. */
int vlgba_triangulate(int m, const double *K, const double *T, const double *w,
                      long long n, const long long *obs_ptr, const int *obs_cam,
                      const double *obs_x, int device, double *X /* 4 x n */,
                      int *status /* n, may be NULL */);

/* One-point refinement with the motion fixed, every point its own problem with
 * its own lambda:
 *   bundle_euclid(K, T, Omega, X_i, x_i, 'fix_calibration', 'fix_motion',
 *                 'visibility', ones(1, k))
 * (replaces bundle_euclid.m:111-249 with mex_bundle_1_XABeUVWeAeB.c:43-70,
 * 196-225, 296-332 and mex_bundle_3_db_new.c:99-166 for n = 1; the LM rule of
 * bundle_euclid.m:205-241 per point on the host, as vlgba_resect applies it).
 * Each point's trajectory equals the CPU restatement's (sequential sums, the
 * closed-form 3 x 3 pseudo-inverse) bit for bit.  X (3 x n) is the start point
 * and receives the result; error_out (n x error_cap, row i = point i's error_,
 * SSE / views per accepted step) and num_error (n) may be NULL.  A point with
 * no views is left untouched, with num_error 0.  opt: max_iter, max_iter2,
 * lambda0, stop_rel, device are honoured (the rest does not apply). */
int vlgba_intersect(int m, const double *K, const double *T, const double *w,
                    long long n, const long long *obs_ptr, const int *obs_cam,
                    const double *obs_x, const vlgba_options *opt,
                    double *X /* 3 x n, start point in, result out */,
                    double *error_out, int error_cap, int *num_error,
                    vlgba_stats *stats);

/* ---- the batched entries with a camera model, a Jacobian mode and a loss -----
 * vlgba_resect, vlgba_intersect and vlgba_triangulate with the capabilities of
 * the fused LM path; those three keep their signatures, refusals and bits.
 *
 * Model.  vlgba_resect_ex accepts prob->num_a 6, 7, 10 and 9 (VLGBA_E_NUMA
 * otherwise).  At 9 the camera has radial distortion exactly as on the fused
 * path: a = [w; T; f; k1; k2], (cx, cy) = K[2], K[3] fixed, K[0], K[1] unused.
 * For the per-point entries a non-NULL kd (2 x m: k1; k2 per camera) makes every
 * camera radial with f = K[0] (K[1] ignored) and (cx, cy) = K[2], K[3]; kd ==
 * NULL is the pinhole model of vlgba_intersect / vlgba_triangulate.  The radial
 * model is analytic only: jacobian == VLGBA_JAC_FD with num_a == 9 or kd != NULL
 * returns VLGBA_E_ARG.
 *
 * Jacobians.  VLGBA_JAC_FD: the reference's forward differences.
 * VLGBA_JAC_ANALYTIC: the closed-form columns of the fused path's analytic mode
 * (the camera columns for resect, B = J R for intersect), for |w| < 1e-6 the
 * limit generators [e_k]x -- a camera handed over at w = 0 rotates, which under
 * forward differences it never does.  The projection is the same in both modes:
 * the residuals, and so the cost at equal parameters, are the same bits.
 * VLGBA_E_ARG for an unknown kind.
 *
 * Loss.  The rules of vlgba_set_loss: w = rho'(s) per observation, its Jacobian
 * rows and residual times sqrt(w) where they are formed, the LM scalars (old /
 * new / dp'(lambda dp + g)) the robust cost and gradient, error_ = cost / views.
 * An observation whose cost is the plain term s itself (no loss; Huber with s <=
 * c^2) is added as the plain pass adds it, so Huber at a scale above every
 * residual gives the bits of VLGBA_LOSS_NONE.  VLGBA_E_ARG for an unknown kind
 * and for a non-finite or <= 0 loss_scale when loss != VLGBA_LOSS_NONE.
 *
 * res_out (2 x N), w_out (N), either may be NULL: the unweighted residuals x -
 * x_hat and the loss's weights (no loss: 1) at the RETURNED parameters, in the
 * caller's observation order (computed once after the last pass).
 *
 * Summation order is that of the plain entries: observations ascending for
 * resect, the views in the given order for intersect, sequentially.  Problem q
 * gives the same bits alone as inside any batch, and two calls the same bits.
 * With VLGBA_JAC_FD, VLGBA_LOSS_NONE and the pinhole model every result equals
 * the plain entry's bit for bit.
 *
 * Not covered: the projective model, the MEX gateways and MATLAB drop-ins,
 * several GPUs, the growing-reconstruction driver (incremental_bundle). */
int vlgba_resect_ex(const vlgba_resect_problem *prob, const vlgba_options *opt,
                    int jacobian /* VLGBA_JAC_* */, int loss /* VLGBA_LOSS_* */,
                    double loss_scale /* pixels */, double *a,
                    double *error_out, int error_cap, int *num_error,
                    double *res_out /* 2 x N or NULL */, double *w_out /* N or NULL */,
                    vlgba_stats *stats);

int vlgba_intersect_ex(int m, const double *K, const double *T, const double *w,
                       const double *kd /* 2 x m (k1; k2) or NULL: pinhole */,
                       long long n, const long long *obs_ptr, const int *obs_cam,
                       const double *obs_x, const vlgba_options *opt,
                       int jacobian, int loss, double loss_scale, double *X,
                       double *error_out, int error_cap, int *num_error,
                       double *res_out, double *w_out, vlgba_stats *stats);

/* vlgba_triangulate under radial lenses.  kd == NULL: vlgba_triangulate itself.
 * Else every measurement x is first undistorted: nd = (x - c) / f, rd = |nd|,
 * r (1 + k1 r^2 + k2 r^4) = rd solved by Newton from r = rd -- at most 20
 * updates, settled when an update changes r by no more than 8 ulps (2^-49 |r|)
 * -- and n = nd (r / rd), n = 0 at rd = 0; then triangulation.m's rows are
 * formed from the pinhole pixel f n + c exactly as vlgba_triangulate forms them,
 * with K = (f, f, cx, cy).  A view fails when the iteration does not settle or
 * when 1 + 3 k1 r^2 + 5 k2 r^4 <= 0 at an iterate or at the settled r (at or
 * past the fold of the lens); a point with such a view gets status 2 and zeros.
 * (A lens whose k2 turns the distortion upwards again beyond the fold has a far
 * branch; an iteration thrown onto it is not detected.) */
int vlgba_triangulate_ex(int m, const double *K, const double *T, const double *w,
                         const double *kd /* 2 x m or NULL */, long long n,
                         const long long *obs_ptr, const int *obs_cam,
                         const double *obs_x, int device, double *X, int *status);

/* Multi-GPU: rank 0 creates the 128-byte RCCL unique id, the caller
 * broadcasts it (e.g. torch.distributed) and passes it as opt->comm_id.
 * NOTE: reuse one id for every solve of a device set, or release each id
 * with vlgba_comm_release once no context will pass it again -- the library
 * keeps the communicators an id made (below); past 64 idle ones it destroys
 * those of the oldest ids, with a warning. */
int vlgba_get_unique_id(void *id128);
/* The library keeps RCCL communicators for the next context created with the
 * same (id, world size, rank).  A caller that will not pass an id again
 * releases it: the idle communicators made from it are destroyed (ones still
 * held by a context are destroyed with it).  Returns the number destroyed. */
int vlgba_comm_release(const void *id128);

/* Diagnostics: the device sin / cos the rotation tables use (glibc's
 * algorithm, vlg_libm.h) for n host arguments -- the parity tests compare them
 * with the host libm bit for bit.  |x| < 105414350. */
int vlgba_debug_sincos(const double *x, double *s, double *c, long long n);
/* the pinv fallback of the reduced solve (rocSOLVER dsyevd + the pinv kernels)
 * on a host ld x ld symmetric S (lower triangle read) and e_: da = pinv(S) e_
 * with MATLAB's tolerance ld * eps(max |eigenvalue|). */
int vlgba_debug_pinv_solve(int ld, const double *S, const double *e_, double *da);
/* Fault injection (tests / the bench's fallback timing): the next `passes`
 * passes of ctx report word 4 = a non-positive pivot (the pass then takes the
 * pinv step) or word 5 = a hand-off spin timeout of the one-launch solve (the
 * pass is solved again without spins), or word 6 = the envelope runner
 * (k_env_runner, opt-in VLGBA_ENV_RUNNER=1) fails to start (the factorization
 * then runs with the column launches alone).  VLGBA_DEBUG_SPIN_TIMEOUT=
 * "rank:passes" sets word 5 at context creation. */
int vlgba_debug_force_status(vlgba_ctx *ctx, int word, int passes);
/* The envelope solve's nested-dissection planner on the host (no GPU): for
 * m cameras of num_a parameters and the co-visible blocks blk_jk [2 * nb]
 * (j >= k), the chosen arc count K (0: none), the arc boundaries bnd [K + 1]
 * (cameras bnd[t] .. bnd[t+1]-1, minus the separator: the cameras co-visible
 * with an earlier arc) and the predicted chain of factor steps (crit).
 * bnd must hold 9 ints. */
int vlgba_debug_nd_plan(int m, int num_a, const int *blk_jk, int nb, int *bnd, int *crit);
/* The plan of the selected inverse (VLGBA_COV_SELECTED) on the host (no GPU),
 * for a cyclic reduction of ntiles >= 1 tiles: the elimination records elim
 * [3 * ntiles] = (e, p, q), p < e < q the kept neighbours or -1, level by level
 * (level l: records eptr[l] .. eptr[l+1]-1; eptr must hold 34 ints), and per
 * record src [2 * ntiles]: the record that holds Sigma_qp and 1 when it is p's
 * (Sigma_qp = Sigma_pq^T of its q side) or 0 when it is q's (its p side as
 * stored); -1, 0 where p or q is absent.  Returns the level count, -1 on bad
 * arguments. */
int vlgba_debug_selinv_plan(int ntiles, int *elim, int *eptr, int *src);
/* The block-Jacobi PCG's structure on the host (no GPU): the reduced system of
 * m cameras as a block CSR over both triangles, from the co-visible blocks
 * blk_jk [2 * nb] (j >= k).  Row j (rowptr [m + 1]) lists its neighbour
 * cameras ascending, the diagonal block among them; entry e is ent[2 e] the
 * block's index and ent[2 e + 1] = 1 when the row reads it transposed (the
 * neighbour is the block's j).  ent must hold 2 * (2 nb) ints.  Returns the
 * entry count nnz, -1 on bad arguments (a pair with j < k, an index outside
 * [0, m), a pair given twice). */
int vlgba_debug_pcg_plan(int m, const int *blk_jk, int nb, int *rowptr, int *ent);

/* Library / device info: writes a NUL-terminated string, returns its length. */
int vlgba_version(char *buf, int len);
/* 0 when abi_version and the sizes of the public structs the caller was
 * compiled with are the library's, else VLGBA_E_ABI (see VLGBA_ABI_VERSION). */
int vlgba_abi_check(int abi_version, long long sz_problem, long long sz_options,
                    long long sz_stats, long long sz_step_info, long long sz_resect_problem);
#define VLGBA_ABI_CHECK()                                                                    \
    vlgba_abi_check(VLGBA_ABI_VERSION, (long long)sizeof(vlgba_problem),                     \
                    (long long)sizeof(vlgba_options), (long long)sizeof(vlgba_stats),        \
                    (long long)sizeof(vlgba_step_info), (long long)sizeof(vlgba_resect_problem))
int vlgba_device_count(void);

/* ---- synthetic scenes on the GPU --------------
 * Configs 2-4's banded model (a restatement of
 * toolbox/test/generate_scene_and_motion.m:36-117: f = width, c = centre,
 * damped random-walk cameras, points at depth U(lo, hi) seen by `track`
 * consecutive cameras, N(0, noise^2) pixel noise) and the perturbation of
 * toolbox/test/demo_bundle_euclid.m:29-31, generated by counter-based
 * (Philox4x32-10) kernels: the same seed gives the same scene on any GPU and
 * launch geometry.  Outputs are host buffers (NULL: not copied); observations
 * are point-major with cameras ascending, N = n * min(track, m).            */
typedef struct {
    int m, n, track;
    double depth_lo, depth_hi;     /* point depth in front of its first camera  */
    double noise;                  /* pixel noise sigma                         */
    unsigned long long seed;
    int keep_first_rotation;       /* w0(:,1) = w(:,1) (the test_mview path)    */
    double width, height;          /* image size; 0 -> 500                      */
} vlgba_scene_spec;

typedef struct {
    double *K, *w, *T, *X;         /* [4m] [3m] [3m] [4n] ground truth (X(4,:) = 1) */
    double *w0, *T0, *X0;          /* [3m] [3m] [4n] perturbed initial values       */
    int *obs_pt, *obs_cam;         /* [N]                                           */
    double *obs_x;                 /* [2N] measured (u, v)                          */
    long long num_obs_cap;         /* capacity of the observation arrays (>= N)     */
    long long num_obs;             /* out: N                                        */
    long long behind;              /* out: observations at depth <= 0.01 depth_lo   */
} vlgba_scene_out;

int vlgba_scene_banded(const vlgba_scene_spec *spec, int device, vlgba_scene_out *out);

#ifdef __cplusplus
}
#endif
#endif /* VLGBA_H */
