// ba_ctx.h -- the solver context (vlgba_ctx) and what the host units share
// (internal): ba_runtime.cpp the process-wide resources, ba_solver.cpp setup,
// the LM pass and most of the C ABI, ba_cov_host.cpp the covariance driver,
// ba_mex.cpp the MEX stage entries.
#pragma once
#include "ba_internal.h"
#include "../../include/vlgba.h"

#include <rccl/rccl.h>
#include <rocsolver/rocsolver.h>   // types only: the library is dlopen'ed on first use

#include <memory>
#include <mutex>
#include <vector>

// internal: none of this is exported from libvlgba.so
#pragma GCC visibility push(hidden)

// ---- ba_runtime.cpp: process-wide resources, nothing of the LM ----
// (ba_dmalloc / ba_dfree / ba_ensure_dyn_lds / kt_begin / kt_end: ba_internal.h)

// totals of the contexts destroyed with timing on: kt_retire adds a context's,
// kt_totals reads them (any pointer may be null) and zeroes them on reset
void kt_retire(const ba_ktimer *kt);
void kt_totals(double *ms, long long *calls, double *flops, int reset);

// a context's streams, fork / join events and host-mapped result block, pooled
// per device: taken for the context's lifetime, returned idle
struct ba_aux {
    int device;
    hipStream_t stream, side;
    hipEvent_t ev_fork, ev_join;
    double *hres_host, *hres_dev;
    double *pin;        // pinned host staging of the plan upload and set_params
    size_t pin_cap;     // its capacity in doubles
};
int aux_acquire(int device, ba_aux &a);
void aux_release(const ba_aux &a);
// the pinned staging grown to at least `doubles`; null if pinned memory is not
// to be had (the caller then copies from pageable memory)
double *aux_pin(ba_aux &a, size_t doubles);

// RCCL communicators outlive their context, keyed by (unique id, world, rank)
ncclResult_t comm_acquire(ncclComm_t *comm, int world, const void *id128, int rank);
void comm_release(ncclComm_t comm);
int comm_forget(const void *id128);   // vlgba_comm_release

// rocSOLVER, loaded on first use (null: not to be had), and one handle per
// device.  A caller holds g_rs_mu while it uses a handle.
struct rs_api {
    rocblas_status (*create)(rocblas_handle *);
    rocblas_status (*set_stream)(rocblas_handle, hipStream_t);
    rocblas_status (*syevd)(rocblas_handle, const rocblas_evect, const rocblas_fill,
                            const rocblas_int, double *, const rocblas_int, double *, double *,
                            rocblas_int *);
    rocblas_status (*potrf)(rocblas_handle, const rocblas_fill, const rocblas_int, double *,
                            const rocblas_int, rocblas_int *);
    rocblas_status (*potrs)(rocblas_handle, const rocblas_fill, const rocblas_int,
                            const rocblas_int, double *, const rocblas_int, double *,
                            const rocblas_int);
    rocblas_status (*potri)(rocblas_handle, const rocblas_fill, const rocblas_int, double *,
                            const rocblas_int, rocblas_int *);
    bool ok = false;
};
rs_api *rs_load();
extern std::mutex g_rs_mu;
int rs_prepare(int device, rs_api **rs_out, rocblas_handle *hdl_out);

// ---- the context ----
// dense scratch of the recovery paths and the dense covariance (ld x ld S, the
// eigenvalues, two work vectors, rocSOLVER's info word), allocated by the first
// ensure() of whoever needs it
struct ba_dense {
    ba_dbuf<double> S, ev, e, w;
    ba_dbuf<int> info;
    int ensure(long long ld);
};

// vlgba_covariance's state (ba_cov_host.cpp), made on the first call that needs
// it: the points binned by track length for k_point_cov (internal order: 8
// lanes | one wave | one workgroup per point), the longest track, the points
// with an observation, the fixed-row mask of S0, the diagonal blocks of Sigma_a
// and Sigma_b
struct ba_cov_state {
    ba_dbuf<int> list;
    int n8 = 0, n64 = 0, nwg = 0, tmax = 0, seen = 0;
    ba_dbuf<unsigned char> fixed;
    ba_dbuf<double> diag, pts;
    // ... and the packed copy of Sigma_a's co-visible blocks k_point_cov reads
    // (CSR by camera row: rowptr [m + 1], col / bj [nb]; VLGBA_COV_PACKED=0:
    // the dense method's kernel reads the dense inverse -- A/B)
    ba_dbuf<int> rowptr, col, bj;
    ba_dbuf<double> packed;
    int src_packed = 1;
    std::vector<int> ord;   // packed block p is block ord[p] of blk_jk
    // the last successful call's blocks are in packed (times scale:
    // vlgba_get_covariance_blocks)
    int have = 0;
    double scale = 1.0;
    // VLGBA_COV_SELECTED (vlgba_set_covariance_method): the selected inverse on
    // the camera-aligned CR factors -- its tile sources and three 32 x 32 tiles
    // per CR tile (allocated on the method's first call)
    int method = VLGBA_COV_DENSE;
    ba_dbuf<int> selsrc;
    ba_dbuf<double> sig;
};

struct vlgba_ctx {
    ba_dev d;
    ba_flags flags;
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    int (*host_allreduce)(double *, long long, void *) = nullptr;
    void *host_user = nullptr;
    int p0 = 0, p1 = 0;          // global point range of this rank
    int n_global = 0;
    long long N_global = 0;
    double num_vis = 0;
    int max_iter = 20, max_iter2 = 10, verbose = 0;
    double lambda = 1e-3, lambda0 = 1e-3, nu = 2.0;
    int model = VLGBA_MODEL_EUCLIDEAN;
    int lin_valid = 0;
    int camred_due = 0;           // fused update: the linearisation swapped in by an
                                  // accepted step still needs its camera reduction
    int timing = 0;
    hipEvent_t ev[8] = {};        // all eight or none (vlgba_set_timing)
    double phase_ms[7] = {};
    std::vector<void *> allocs;
    std::vector<double> hb_tmp;   // host staging for b gather
    ba_aux aux;                   // streams / events / host result block (pooled)
    bool has_aux = false;
    double stop_rel = 1e-3;       // bundle_euclid.m:123 relative-decrease stop
    void (*on_pass)(int, int, const vlgba_step_info *, void *) = nullptr;
    void *on_pass_user = nullptr;
    // internal point order (fast path, one rank): the short-track points that
    // fit the MFMA Schur chunks first, then the rest, each in input order.
    // pperm[new] = input point, operm[new obs] = input observation (point-major
    // input order), both relative to this rank's first point / observation;
    // empty = identity.
    std::vector<int> pperm, operm;
    ba_dense dense;               // pinv_fallback, nd_natural_retry, dense covariance
    int pinv_used = 0;            // passes that took the pinv fallback
    int nd_retries = 0;           // nested-dissection pivots solved in the natural order
    int spin_retries = 0;         // passes re-solved after a hand-off timeout
    int debug_timeouts = 0;       // test hooks: passes whose timeout word / pivot word
    int debug_pivots = 0;         // is forced (vlgba_debug_force_status)
    std::unique_ptr<ba_cov_state> cov;
};

// ---- ba_solver.cpp ----
int ctx_create(const vlgba_problem *p, const vlgba_options *o, vlgba_ctx **out, bool lower_blocks,
               bool all_diag, bool stage_mode);
void ctx_free(vlgba_ctx *c);
// owner of a context on the paths that make one for a single call
struct ctx_deleter {
    void operator()(vlgba_ctx *c) const { ctx_free(c); }
};
using ctx_ptr = std::unique_ptr<vlgba_ctx, ctx_deleter>;

// device memory that lives as long as the context
template <typename T>
inline int ctx_alloc(vlgba_ctx *c, T **p, size_t count)
{
    TRY_RC(dalloc(p, count));
    c->allocs.push_back((void *)*p);
    return 0;
}

// every handle entry point runs on the context's device, whatever the calling
// thread's current device is (allocations and launches follow hipGetDevice)
inline int ctx_enter(vlgba_ctx *c)
{
    return hipSetDevice(c->aux.device) == hipSuccess ? 0 : VLGBA_E_ARG;
}

// where stage 1 runs the camera reduction
enum camred_route {
    CAMRED_PLAIN,   // its own launch on the library stream
    CAMRED_SIDE,    // its own launch on the side stream, beside V*^-1 and the Schur
                    // chunks of the Schur phase that follows
    CAMRED_FOLD     // workgroups of the MFMA Schur launch that follows
};
// what stage 1 left for the Schur phase of the same pass (CAMRED_SIDE,
// CAMRED_FOLD); the default: nothing
struct stage1_left {
    bool fold = false;          // run the reduction fold_args inside the MFMA Schur launch
    ba_camred fold_args{};
    bool side_camred = false;   // join the side stream before k_schur_reduce
};
int stage1(vlgba_ctx *c, int relinearize, camred_route route, stage1_left *left);
int schur_phase(vlgba_ctx *c, double lam, const stage1_left &left = {});
// per-point device array (k doubles per local point, internal order) -> host,
// in the input point order (synchronous when a permutation applies)
int download_points(vlgba_ctx *c, double *dst, const double *src, int k);
// dpotrf / dpotri (fn) on the lower triangle of the dense scratch, in place,
// and its info word on the host.  The caller holds g_rs_mu and has set the
// handle's stream.
int rs_factor_info(vlgba_ctx *c, rocblas_handle hdl, decltype(rs_api::potrf) fn, int *info);

#pragma GCC visibility pop
