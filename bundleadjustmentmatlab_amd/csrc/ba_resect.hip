// ba_resect.hip -- batched one-camera bundle adjustment with the structure
// fixed: the non-linear refinement of estimate_camera.m:247-253,
//     [K T Omega] = bundle_euclid(K, T, Omega, X, x0, 'fix_calibration',
//                                 'fix_structure', 'visibility', inlier')
// (or without 'fix_calibration' for an uncalibrated camera), for many cameras
// at once (growing BA adds one camera per step and resects it; a whole batch of
// views can be resected against one structure).
//
// With m = 1 and 'fix_structure' the reference's pass (bundle_euclid.m:120-249)
// reduces exactly to: mex_bundle_1 for the camera's columns of A and e
// (mex_bundle_1_XABeUVWeAeB.c:192-256, 266-290, 317-323), the fix mask zeroing
// V, W, eB (bundle_euclid.m:140-144) so that V*^-1 = pinv(0) = 0, Y = 0,
// S = U* and e_ = eA - 0 (mex_bundle_2_Se_.c), da = pinv(S) e_ (:193), db = 0 and
// b unchanged (mex_bundle_3_db_new.c:99-146), the new projections, e'e and
// dp'(lambda dp + g) with the point entries exact zeros.  Every sum here runs
// sequentially in the reference's order (observations ascending) and the 6 x 6
// (num_a x num_a) solve is the parity-mode sequential Cholesky (pinv by cyclic
// Jacobi on a non-positive pivot: ba_small_solve.h, host and device; such a
// pass counts in vlgba_stats.pinv_passes), so each problem's trajectory equals
// the oracle's bundle_euclid restatement with m = 1 (vinv formula, solve / sums
// sequential) bit for bit.
//
// One workgroup per camera and LM pass: observations in tiles of 256 (one lane
// each: projection + num_a forward-difference columns into LDS), then
// NA*NA + NA + 1 accumulator lanes walk the tile in order.  The LM control
// (bundle_euclid.m:205-241, glibc pow for the lambda rule) stays on the host,
// per problem, exactly as vlgba_run applies it: the driver of ba_batch_lm.h on
// the device backend of ba_batch_dev.h, both shared with the per-point dual
// vlgba_intersect of ba_triang.hip.  resect_run checks the arguments, uploads
// the problem and hands over a launch and a residual lambda.
//
// vlgba_resect_ex (include/vlgba.h) runs the same pass with the fused path's
// analytic Jacobians, radial-distortion camera (num_a = 9) and robust losses:
// further instantiations of k_resect_pass (below), the same host control.
#include "ba_camera.h"
#include "ba_batch_dev.h"
#include "ba_small_solve.h"
#include "../../include/vlgba.h"

#include <chrono>
#include <cstring>
#include <type_traits>

#define RS_TILE 256

// state per problem: U (NA x NA) | eA (NA) | old SSE, kept across rejected
// passes (bundle_euclid.m:139 recomputes an identical linearisation, Q12)
//
// The modes of vlgba_resect_ex.  JAC: the closed-form camera columns of
// cam_view<NA>::jac_columns (one evaluation per observation instead of NA + 1
// projections) from the table R(w), dR/dw_k of rotations5_jac; the projection,
// and with it every residual and the cost at equal parameters, is the FD
// mode's bit for bit.  NA = BA_RAD_NA (radial lens) exists with JAC alone.
// LOSS: the observation's row [A | e] times sqrt(w) where it is formed
// (vlg_loss), the old / new cost sum rho(s) in observation order -- a plain
// term (vlg_loss_plain) added as the plain pass adds it -- and the gradient of
// dp'(lambda dp + g) the weighted eA: the rules of vlgba_set_loss.  The row then
// carries the observation's two cost terms in two more columns, formed by its
// own lane: the accumulator lanes' serial walk over the tile is what a pass
// waits for, and it stays two loads and two adds per observation.
// <NA, false, false> is vlgba_resect's pass.  LDS at the widest row (NA = 10,
// LOSS): 256 x 25 doubles = 50 KB of At and under 3 KB of the rest.
template <int NA>
__device__ __forceinline__ void resect_project_new(const double *k4, const double *an,
                                                   const double *rotn, const double b[3],
                                                   double xh[2])
{
    if constexpr (NA == BA_RAD_NA) {
        vlg_project_radial(an + 6, k4 + 2, rotn, an + 3, b, xh);
    } else {
        double Kc[9];
        vlg_calib(Kc, k4, an, NA - 6);
        vlg_project(Kc, rotn, an + 3, b, xh);
    }
}

// Under a loss: the two terms t[0], t[1] the cost lane adds for the residual
// (e0, e1), so that its serial loop stays free of branches -- a plain term's
// e0 e0 and e1 e1, as the plain pass adds them, else rho and an exact + 0.
// Returns sqrt(w).
__device__ __forceinline__ double resect_cost_terms(ba_loss ls, double e0, double e1, double *t)
{
    const double s = e0 * e0 + e1 * e1;
    double rho, sw;
    vlg_loss(ls.kind, ls.c, s, &rho, &sw);
    const bool plain = vlg_loss_plain(ls.kind, ls.c, s);
    t[0] = plain ? e0 * e0 : rho;
    t[1] = plain ? e1 * e1 : 0.0;
    return sw;
}

template <int NA, bool JAC, bool LOSS>
__global__ __launch_bounds__(256) void k_resect_pass(
    int nprob, const long long *__restrict__ obs_ptr, const double *__restrict__ Xw,
    const double *__restrict__ xo, const double *__restrict__ K4, double *__restrict__ a,
    double *__restrict__ a_new, double *__restrict__ state, const double *__restrict__ lam_p,
    const double *__restrict__ flags, double *__restrict__ out, ba_loss ls)
{
    static_assert(JAC || NA != BA_RAD_NA, "the radial model is analytic only");
    constexpr int NUE = NA * NA + NA + 1;
    // LOSS: two cost terms more, and a pad that keeps the row stride odd
    constexpr int RW = 2 * NA + 2 + (LOSS ? 3 : 0);
    __shared__ double rot[45], rotn[9], k4[4], av[NA], an[NA];
    __shared__ double At[RS_TILE][RW];     // A (2 x NA, column major) | e (| cost terms)
    __shared__ double st[NUE], S[NA * NA], rhs[NA], da[NA];
    __shared__ int fail;
    const int pb = blockIdx.x, tid = threadIdx.x;
    if (pb >= nprob) return;
    // staged with lambda as doubles (one copy a pass); a vector load at device
    // scope, as every per-pass word (ba_internal.h)
    const int fl = (int)__hip_atomic_load(flags + pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!(fl & 1)) return;                          // problem finished
    const long long o0 = obs_ptr[pb], no = obs_ptr[pb + 1] - o0;
    double *stg = state + (size_t)NUE * pb;
    if (tid < NA) {
        if (fl & 4) a[(size_t)NA * pb + tid] = a_new[(size_t)NA * pb + tid];   // accepted
    }
    if (tid < 4) k4[tid] = K4[4 * (size_t)pb + tid];
    __syncthreads();
    if (tid < NA) av[tid] = a[(size_t)NA * pb + tid];
    if (tid == 0) fail = 0;
    __syncthreads();
    if (fl & 2) {   // linearise at a (mex_bundle_1 for this camera)
        if (tid == 0) {
            const double w[3] = {av[0], av[1], av[2]};
            if constexpr (JAC) rotations5_jac(w, rot);
            else rotations5(w, rot);
        }
        double acc = 0.0;   // lane q < NUE: U[q] | eA[q - NA^2] | old SSE
        __syncthreads();
        const cam_view<NA> cv(av, k4, rot, 0);
        for (long long t0 = 0; t0 < no; t0 += RS_TILE) {
            const int nt = (int)(no - t0 < RS_TILE ? no - t0 : RS_TILE);
            if (tid < nt) {
                const long long o = o0 + t0 + tid;
                const double b[3] = {Xw[3 * o], Xw[3 * o + 1], Xw[3 * o + 2]};
                double xh[2];
                cv.project(b, xh);
                double *row = At[tid];
                if constexpr (JAC) {
                    // both halves of the closed form; its point columns (the six
                    // entries past 2 NA) are not stored
                    double jr[2 * NA + 6];
                    cv.jac_columns(b, 0, jr);
                    cv.jac_columns(b, 1, jr);
#pragma unroll
                    for (int k = 0; k < 2 * NA; k++) row[k] = jr[k];
                } else {
#pragma unroll 1
                    for (int k = 0; k < NA; k++) {   // derivative_camera (:14-41)
                        double x1[2];
                        cv.project_dcam(k, b, x1);
                        row[2 * k] = vlg_fd_quot(x1[0] - xh[0]);
                        row[2 * k + 1] = vlg_fd_quot(x1[1] - xh[1]);
                    }
                }
                row[2 * NA] = xo[2 * o] - xh[0];          // e = X - X_hat (:222-223)
                row[2 * NA + 1] = xo[2 * o + 1] - xh[1];
                if constexpr (LOSS) {
                    const double sw = resect_cost_terms(ls, row[2 * NA], row[2 * NA + 1],
                                                        row + 2 * NA + 2);
#pragma unroll 1
                    for (int k = 0; k < 2 * NA + 2; k++) row[k] *= sw;
                }
            }
            __syncthreads();
            if (tid < NA * NA) {                  // U += A'A, entry (r, c) (:281-290)
                const int r = tid % NA, c = tid / NA;
                for (int q = 0; q < nt; q++)
                    acc += At[q][2 * r] * At[q][2 * c] + At[q][2 * r + 1] * At[q][2 * c + 1];
            } else if (tid < NA * NA + NA) {      // eA += A'e (:317-323)
                const int r = tid - NA * NA;
                for (int q = 0; q < nt; q++)
                    acc += At[q][2 * r] * At[q][2 * NA] + At[q][2 * r + 1] * At[q][2 * NA + 1];
            } else if (tid == NUE - 1) {          // e(:)'e(:) in MATLAB's flat order
                for (int q = 0; q < nt; q++) {
                    if constexpr (LOSS) {
                        acc = acc + At[q][2 * NA + 2];
                        acc = acc + At[q][2 * NA + 3];
                    } else {
                        acc = acc + At[q][2 * NA] * At[q][2 * NA];
                        acc = acc + At[q][2 * NA + 1] * At[q][2 * NA + 1];
                    }
                }
            }
            __syncthreads();
        }
        if (tid < NUE) stg[tid] = acc;
    }
    __syncthreads();
    if (tid < NUE) st[tid] = stg[tid];
    __syncthreads();
    const double lambda = __hip_atomic_load(lam_p + pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // S = U* (damped diagonal), e_ = eA, da = pinv(S) e_: ba_small_solve.h
    if (tid == 0 && small_solve_damped<NA>(st, lambda, S, rhs, da)) fail = 1;
    __syncthreads();
    if (tid < NA) {   // a_new = a + da (mex_bundle_3_db_new.c:137-140)
        an[tid] = av[tid] + da[tid];
        a_new[(size_t)NA * pb + tid] = an[tid];
    }
    __syncthreads();
    if (tid == 0) {
        const double w[3] = {an[0], an[1], an[2]};
        vlg_rodrigues(rotn, w);
    }
    __syncthreads();
    // new projections (:149-166; b_new = b + db with db = 0), then e_new'e_new
    double nsum = 0.0;
    for (long long t0 = 0; t0 < no; t0 += RS_TILE) {
        const int nt = (int)(no - t0 < RS_TILE ? no - t0 : RS_TILE);
        if (tid < nt) {
            const long long o = o0 + t0 + tid;
            const double b[3] = {Xw[3 * o], Xw[3 * o + 1], Xw[3 * o + 2]};
            double xh[2];
            resect_project_new<NA>(k4, an, rotn, b, xh);
            const double e0 = xo[2 * o] - xh[0], e1 = xo[2 * o + 1] - xh[1];
            if constexpr (LOSS) {
                (void)resect_cost_terms(ls, e0, e1, At[tid]);
            } else {
                At[tid][0] = e0;
                At[tid][1] = e1;
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int q = 0; q < nt; q++) {
                if constexpr (LOSS) {
                    nsum = nsum + At[q][0];
                    nsum = nsum + At[q][1];
                } else {
                    nsum = nsum + At[q][0] * At[q][0];
                    nsum = nsum + At[q][1] * At[q][1];
                }
            }
        __syncthreads();
    }
    if (tid == 0) {
        double g = 0.0;   // dp'(lambda dp + g): the point entries are exact zeros
        for (int k = 0; k < NA; k++) g = g + da[k] * (lambda * da[k] + st[NA * NA + k]);
        out[4 * (size_t)pb + 0] = st[NUE - 1];
        out[4 * (size_t)pb + 1] = nsum;
        out[4 * (size_t)pb + 2] = g;
        out[4 * (size_t)pb + 3] = fail ? 1.0 : 0.0;
    }
}

// res_out / w_out of vlgba_resect_ex: the unweighted residuals x - x_hat and the
// loss's weights (sqrt(w) squared; 1 without a loss) at the returned parameters
// a, one workgroup per camera; either pointer may be NULL
template <int NA>
__global__ __launch_bounds__(256) void k_resect_residuals(
    int nprob, const long long *__restrict__ obs_ptr, const double *__restrict__ Xw,
    const double *__restrict__ xo, const double *__restrict__ K4, const double *__restrict__ a,
    ba_loss ls, double *__restrict__ res, double *__restrict__ wt)
{
    __shared__ double rotn[9], k4[4], av[NA];
    const int pb = blockIdx.x, tid = threadIdx.x;
    if (pb >= nprob) return;
    if (tid < NA) av[tid] = a[(size_t)NA * pb + tid];
    if (tid < 4) k4[tid] = K4[4 * (size_t)pb + tid];
    __syncthreads();
    if (tid == 0) {
        const double w[3] = {av[0], av[1], av[2]};
        vlg_rodrigues(rotn, w);
    }
    __syncthreads();
    for (long long o = obs_ptr[pb] + tid; o < obs_ptr[pb + 1]; o += 256) {
        const double b[3] = {Xw[3 * o], Xw[3 * o + 1], Xw[3 * o + 2]};
        double xh[2], rho, sw;
        resect_project_new<NA>(k4, av, rotn, b, xh);
        const double e0 = xo[2 * o] - xh[0], e1 = xo[2 * o + 1] - xh[1];
        vlg_loss(ls.kind, ls.c, e0 * e0 + e1 * e1, &rho, &sw);
        if (res) {
            res[2 * o] = e0;
            res[2 * o + 1] = e1;
        }
        if (wt) wt[o] = sw * sw;
    }
}

namespace {
// f(std::integral_constant<int, NA>) at the runtime num_a, or VLGBA_E_ARG
template <class F>
int rs_dispatch_na(int na, F &&f)
{
    switch (na) {
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 10: return f(std::integral_constant<int, 10>());
    case BA_RAD_NA: return f(std::integral_constant<int, BA_RAD_NA>());
    default: return VLGBA_E_ARG;
    }
}

// the pass of one mode at the runtime num_a
struct rs_args {
    int np;
    const long long *ptr;
    const double *X, *x, *K;
    double *a, *an, *st;
    const double *lam, *fl;
    double *out;
    ba_loss ls;
};

// 0, or VLGBA_E_ARG for a (num_a, mode) pair that has no kernel (the radial
// model under forward differences): nothing is launched then
template <bool JAC, bool LOSS>
int rs_launch_na(int na, const rs_args &g, hipStream_t s)
{
    return rs_dispatch_na(na, [&](auto c) {
        constexpr int NA = decltype(c)::value;
        if constexpr (JAC || NA != BA_RAD_NA) {
            k_resect_pass<NA, JAC, LOSS><<<g.np, 256, 0, s>>>(
                g.np, g.ptr, g.X, g.x, g.K, g.a, g.an, g.st, g.lam, g.fl, g.out, g.ls);
            return 0;
        } else {
            return (int)VLGBA_E_ARG;
        }
    });
}

int rs_launch(int na, bool jac, const rs_args &g, hipStream_t s)
{
    if (jac) return g.ls.kind ? rs_launch_na<true, true>(na, g, s)
                              : rs_launch_na<true, false>(na, g, s);
    return g.ls.kind ? rs_launch_na<false, true>(na, g, s) : rs_launch_na<false, false>(na, g, s);
}

// vlgba_resect (ex false: num_a 6 / 7 / 10, forward differences, no loss) and
// vlgba_resect_ex
int resect_run(const vlgba_resect_problem *pr, const vlgba_options *opt, bool ex, int jacobian,
               ba_loss ls, double *a, double *error_out, int error_cap, int *num_error,
               double *res_out, double *w_out, vlgba_stats *stats)
{
    if (!pr || !a || pr->nprob < 0 || !pr->obs_ptr || (error_out && error_cap < 0))
        return VLGBA_E_ARG;
    const int na = pr->num_a, np = pr->nprob;
    if (na != 6 && na != 7 && na != 10 && !(ex && na == BA_RAD_NA)) return VLGBA_E_NUMA;
    if (ex)
        if (int rc = batch_check_mode(jacobian, ls.kind, ls.c, na == BA_RAD_NA)) return rc;
    if (ls.kind == VLGBA_LOSS_NONE) ls.c = 0.0;
    if (np == 0) return 0;
    const long long N = pr->obs_ptr[np];
    if (pr->obs_ptr[0] != 0 || N < 0 || (N > 0 && (!pr->X || !pr->x)) || !pr->K)
        return VLGBA_E_ARG;
    for (int q = 0; q < np; q++)
        if (pr->obs_ptr[q + 1] < pr->obs_ptr[q]) return VLGBA_E_ARG;
    vlgba_options dflt;
    std::memset(&dflt, 0, sizeof dflt);
    if (!opt) opt = &dflt;
    VLGBA_CHECK(hipSetDevice(opt->device));
    const auto t0 = std::chrono::steady_clock::now();
    // before the stream's guard: freed after it has drained (ba_batch_dev.h)
    ba_dbuf<long long> d_ptr;
    ba_dbuf<double> d_X, d_x, d_K, d_st, d_res;
    batch_stream bs(opt->device, 6 * (size_t)np);
    if (bs.rc) return bs.rc;
    hipStream_t s = bs.s;
    TRY_RC(d_ptr.alloc((size_t)np + 1));
    TRY_RC(d_X.alloc(3 * (size_t)N));
    TRY_RC(d_x.alloc(2 * (size_t)N));
    TRY_RC(d_K.alloc(4 * (size_t)np));
    TRY_RC(d_st.alloc((size_t)(na * na + na + 1) * np));   // U | eA | old cost per problem
    TRY_RC(upload(d_ptr.get(), pr->obs_ptr, (size_t)np + 1, s));
    TRY_RC(upload(d_X.get(), pr->X, 3 * (size_t)N, s));
    TRY_RC(upload(d_x.get(), pr->x, 2 * (size_t)N, s));
    TRY_RC(upload(d_K.get(), pr->K, 4 * (size_t)np, s));
    batch_lm lm((size_t)np, opt);   // the LM control, per problem (ba_batch_lm.h)
    const batch_dev_fn pass = [&](const batch_dev_io &d) {
        return rs_launch(na, jacobian == VLGBA_JAC_ANALYTIC,
                         rs_args{np, d_ptr, d_X, d_x, d_K, d.x, d.x_new, d_st, d.lam, d.flags,
                                 d.out, ls},
                         s);
    };
    batch_dev_fn residuals;
    if (N > 0 && (res_out || w_out))
        residuals = [&](const batch_dev_io &d) {
            TRY_RC(d_res.alloc(3 * (size_t)N));
            double *d_w = d_res + 2 * (size_t)N;
            TRY_RC(rs_dispatch_na(na, [&](auto c) {
                k_resect_residuals<decltype(c)::value><<<np, 256, 0, s>>>(
                    np, d_ptr, d_X, d_x, d_K, d.x, ls, d_res, d_w);
                return -(int)hipGetLastError();
            }));
            if (res_out) TRY_RC(download(res_out, d_res.get(), 2 * (size_t)N, s));
            if (w_out) TRY_RC(download(w_out, d_w, (size_t)N, s));
            return 0;
        };
    return batch_dev_run(bs, lm, na, pr->obs_ptr, a, error_out, error_cap, num_error, stats, t0,
                         pass, residuals);
}
}   // namespace

extern "C" int vlgba_resect(const vlgba_resect_problem *pr, const vlgba_options *opt, double *a,
                            double *error_out, int error_cap, int *num_error,
                            vlgba_stats *stats)
{
    return resect_run(pr, opt, false, VLGBA_JAC_FD, ba_loss{VLGBA_LOSS_NONE, 0.0}, a, error_out,
                      error_cap, num_error, nullptr, nullptr, stats);
}

extern "C" int vlgba_resect_ex(const vlgba_resect_problem *pr, const vlgba_options *opt,
                               int jacobian, int loss, double loss_scale, double *a,
                               double *error_out, int error_cap, int *num_error, double *res_out,
                               double *w_out, vlgba_stats *stats)
{
    return resect_run(pr, opt, true, jacobian, ba_loss{loss, loss_scale}, a, error_out, error_cap,
                      num_error, res_out, w_out, stats);
}
