// ba_triang.hip -- the per-point half of adding a view, batched: linear
// triangulation (triangulation.m:19-53 of the reference's toolbox/geometry) and
// the one-point bundle adjustment with the motion fixed,
//     bundle_euclid(K, T, Omega, X_i, x_i, 'fix_calibration', 'fix_motion',
//                   'visibility', ones(1, k))
// for every point i as its own problem with its own lambda -- the mirror image
// of ba_resect.hip (one camera, structure fixed).  Pinhole Euclidean model.
//
// With n = 1 and 'fix_motion' the reference's pass (bundle_euclid.m:120-249)
// reduces exactly to: mex_bundle_1 for the point's columns of B and e
// (mex_bundle_1_XABeUVWeAeB.c:43-70, 196-225), V = sum B'B and eB = sum B'e in
// view order (:296-332), the fix mask zeroing U, W, eA (bundle_euclid.m:145-149)
// so that S = 0, da = pinv(0) = 0 and e_ = 0, V* damped (:162-184), db =
// V*^-1 eB (mex_bundle_3_db_new.c:99-134 subtracts exact zeros), the new
// projections, e(:)'e(:) in MATLAB's flat order and dp'(lambda dp + g) with the
// camera entries exact zeros.  One lane per point runs the whole pass
// sequentially over its views, which is the reference's summation order, so
// each point's trajectory equals the oracle's bundle_euclid restatement with
// n = 1 (vinv formula, solve / sums sequential) bit for bit.
//
// Both entries first form one record per camera (k_tri_cameras: R(w) by the
// project's Rodrigues with the device sin / cos of vlg_libm.h, as the rotation
// tables use, and P = calibration_matrix(K) [R T]); the point columns of the
// forward differences use the unperturbed camera (mex_bundle_1 :59-66), so
// R(w) is the only one of the table's five rotations a pass reads.
//
// Geometry: a wave per workgroup, one lane per point, so that a batch of a few
// hundred points still spreads over CUs.  The arithmetic is ba_triang_math.h
// (host and device); the working set of a lane stays in registers.
//
// vlgba_triangulate_ex / vlgba_intersect_ex (include/vlgba.h) add the radial
// lens (k1, k2 per camera in a side array next to the unchanged records; the
// undistortion before triangulation.m's rows), the closed-form B and the robust
// losses: k_triangulate_radial, and k_intersect_pass<true> beside the plain
// entry's k_intersect_pass<false>, in which the mode folds away.
#include "ba_batch_lm.h"
#include "ba_internal.h"
#include "ba_triang_math.h"

#define TRI_WAVE 64

__global__ __launch_bounds__(TRI_WAVE) void k_tri_cameras(int m, const double *__restrict__ K,
                                                          const double *__restrict__ T,
                                                          const double *__restrict__ w,
                                                          int radial,
                                                          double *__restrict__ rec)
{
    const int j = blockIdx.x * TRI_WAVE + threadIdx.x;
    if (j >= m) return;
    // radial lenses: K = (f, f, cx, cy) with f = K[0], K[1] ignored
    const double k4[4] = {K[4 * (size_t)j], K[4 * (size_t)j + (radial ? 0 : 1)],
                          K[4 * (size_t)j + 2], K[4 * (size_t)j + 3]};
    const double t[3] = {T[3 * (size_t)j], T[3 * (size_t)j + 1], T[3 * (size_t)j + 2]};
    const double om[3] = {w[3 * (size_t)j], w[3 * (size_t)j + 1], w[3 * (size_t)j + 2]};
    double r[TRI_CAM];
    tri_camera(k4, t, om, r);
#pragma unroll
    for (int c = 0; c < TRI_CAM; c++) rec[(size_t)TRI_CAM * j + c] = r[c];
}

__global__ __launch_bounds__(TRI_WAVE) void k_triangulate(long long n,
                                                          const long long *__restrict__ obs_ptr,
                                                          const int *__restrict__ obs_cam,
                                                          const double *__restrict__ obs_x,
                                                          const double *__restrict__ rec,
                                                          double *__restrict__ X,
                                                          int *__restrict__ status)
{
    const long long i = (long long)blockIdx.x * TRI_WAVE + threadIdx.x;
    if (i >= n) return;
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    double x[4];
    const int st = tri_point(nv, obs_cam + o0, obs_x + 2 * o0, rec, x);
    X[4 * i] = x[0];
    X[4 * i + 1] = x[1];
    X[4 * i + 2] = x[2];
    X[4 * i + 3] = x[3];
    status[i] = st;
}

// ---- the entries with a mode (vlgba_triangulate_ex, vlgba_intersect_ex) -------
// k_triangulate under radial lenses: every measurement undistorted first
// (tri_point_radial)
__global__ __launch_bounds__(TRI_WAVE) void k_triangulate_radial(
    long long n, const long long *__restrict__ obs_ptr, const int *__restrict__ obs_cam,
    const double *__restrict__ obs_x, const double *__restrict__ rec,
    const double *__restrict__ kd, double *__restrict__ X, int *__restrict__ status)
{
    const long long i = (long long)blockIdx.x * TRI_WAVE + threadIdx.x;
    if (i >= n) return;
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    double x[4];
    const int st = tri_point_radial(nv, obs_cam + o0, obs_x + 2 * o0, rec, kd, x);
    X[4 * i] = x[0];
    X[4 * i + 1] = x[1];
    X[4 * i + 2] = x[2];
    X[4 * i + 3] = x[3];
    status[i] = st;
}

// state per point (SoA, entry k of point i at state[k * n + i]): V | eB | old
// cost, kept across rejected passes (bundle_euclid.m:139 recomputes an identical
// linearisation, Q12), as k_resect_pass keeps U | eA | old cost.  M = false:
// vlgba_intersect's pass (md is not read); M = true: the mode md of
// vlgba_intersect_ex, wave-uniform (the radial projection, the closed-form B,
// the loss: the robust cost in place of the SSE)
template <bool M>
__global__ __launch_bounds__(TRI_WAVE) void k_intersect_pass(
    long long n, const long long *__restrict__ obs_ptr, const int *__restrict__ obs_cam,
    const double *__restrict__ obs_x, const double *__restrict__ rec, isect_mode md,
    double *__restrict__ b, double *__restrict__ b_new, double *__restrict__ state,
    const double *__restrict__ lam_p, const double *__restrict__ flags, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * TRI_WAVE + threadIdx.x;
    if (i >= n) return;
    // staged with lambda as doubles (one copy a pass); a vector load at device
    // scope, as every per-pass word (ba_internal.h)
    const int fl = (int)__hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!(fl & 1)) return;                          // point finished (or without views)
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    const int *cam = obs_cam + o0;
    const double *x = obs_x + 2 * o0;
    double bv[3], st[TRI_NST];
    if (fl & 4) {
#pragma unroll
        for (int c = 0; c < 3; c++) b[3 * i + c] = b_new[3 * i + c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) bv[c] = b[3 * i + c];
    if (fl & 2) {
        isect_linearize<M>(nv, cam, x, rec, &md, bv, st);
#pragma unroll
        for (int k = 0; k < TRI_NST; k++) state[(size_t)k * n + i] = st[k];
    } else {
#pragma unroll
        for (int k = 0; k < TRI_NST; k++) st[k] = state[(size_t)k * n + i];
    }
    const double lambda = __hip_atomic_load(lam_p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double bn[3], nsum, g;
    isect_step<M>(nv, cam, x, rec, &md, bv, st, lambda, bn, &nsum, &g);
#pragma unroll
    for (int c = 0; c < 3; c++) b_new[3 * i + c] = bn[c];
    out[4 * i + 0] = st[12];
    out[4 * i + 1] = nsum;
    out[4 * i + 2] = g;
    out[4 * i + 3] = 0.0;
}

// res_out / w_out of vlgba_intersect_ex at the returned points b; either may
// be NULL
__global__ __launch_bounds__(TRI_WAVE) void k_intersect_residuals(
    long long n, const long long *__restrict__ obs_ptr, const int *__restrict__ obs_cam,
    const double *__restrict__ obs_x, const double *__restrict__ rec, isect_mode md,
    const double *__restrict__ b, double *__restrict__ res, double *__restrict__ w)
{
    const long long i = (long long)blockIdx.x * TRI_WAVE + threadIdx.x;
    if (i >= n) return;
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    const double bv[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]};
    isect_residuals_m(nv, obs_cam + o0, obs_x + 2 * o0, rec, &md, bv, res ? res + 2 * o0 : nullptr,
                      w ? w + o0 : nullptr);
}

namespace {
template <typename T>
int dmalloc_n(T **p, size_t n)
{
    *p = (T *)ba_dmalloc(sizeof(T) * (n ? n : 1));
    return *p ? 0 : -(int)hipErrorOutOfMemory;
}

// the argument rules both entries share, before any device work
int check_tracks(int m, const double *K, const double *T, const double *w, long long n,
                 const long long *obs_ptr, const int *obs_cam, const double *obs_x,
                 const double *X)
{
    if (m < 1 || n < 0 || !K || !T || !w || !obs_ptr || (!X && n > 0)) return VLGBA_E_ARG;
    if (obs_ptr[0] != 0) return VLGBA_E_ARG;
    for (long long i = 0; i < n; i++)
        if (obs_ptr[i + 1] < obs_ptr[i]) return VLGBA_E_ARG;
    const long long N = obs_ptr[n];
    if (N > 0 && (!obs_cam || !obs_x)) return VLGBA_E_ARG;
    for (long long o = 0; o < N; o++)
        if (obs_cam[o] < 0 || obs_cam[o] >= m) return VLGBA_E_ARG;
    return 0;
}

// device copies of the cameras' records and the tracks
struct tri_dev {
    long long *ptr = nullptr;
    int *cam = nullptr;
    double *x = nullptr, *in = nullptr, *rec = nullptr;
    double *kd = nullptr;   // k1, k2 per camera (in + 10 m) or null: pinhole
    ~tri_dev()
    {
        for (void *p : {(void *)ptr, (void *)cam, (void *)x, (void *)in, (void *)rec})
            if (p) ba_dfree(p);
    }
    int upload(int m, const double *K, const double *T, const double *w, long long n,
               const long long *obs_ptr, const int *obs_cam, const double *obs_x, hipStream_t s,
               const double *kd_host = nullptr)
    {
        const long long N = obs_ptr[n];
        int rc;
        if ((rc = dmalloc_n(&ptr, (size_t)n + 1)) || (rc = dmalloc_n(&cam, (size_t)N)) ||
            (rc = dmalloc_n(&x, 2 * (size_t)N)) || (rc = dmalloc_n(&in, 12 * (size_t)m)) ||
            (rc = dmalloc_n(&rec, (size_t)TRI_CAM * m)))
            return rc;
        if (hipMemcpyAsync(ptr, obs_ptr, sizeof(long long) * (n + 1), hipMemcpyHostToDevice, s) !=
                hipSuccess ||
            (N > 0 && (hipMemcpyAsync(cam, obs_cam, sizeof(int) * N, hipMemcpyHostToDevice, s) !=
                           hipSuccess ||
                       hipMemcpyAsync(x, obs_x, sizeof(double) * 2 * N, hipMemcpyHostToDevice,
                                      s) != hipSuccess)) ||
            hipMemcpyAsync(in, K, sizeof(double) * 4 * m, hipMemcpyHostToDevice, s) !=
                hipSuccess ||
            hipMemcpyAsync(in + 4 * (size_t)m, T, sizeof(double) * 3 * m, hipMemcpyHostToDevice,
                           s) != hipSuccess ||
            hipMemcpyAsync(in + 7 * (size_t)m, w, sizeof(double) * 3 * m, hipMemcpyHostToDevice,
                           s) != hipSuccess)
            return -1;
        if (kd_host) {
            kd = in + 10 * (size_t)m;
            if (hipMemcpyAsync(kd, kd_host, sizeof(double) * 2 * m, hipMemcpyHostToDevice, s) !=
                hipSuccess)
                return -1;
        }
        k_tri_cameras<<<(m + TRI_WAVE - 1) / TRI_WAVE, TRI_WAVE, 0, s>>>(
            m, in, in + 4 * (size_t)m, in + 7 * (size_t)m, kd_host != nullptr, rec);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
};

// vlgba_triangulate (kd null: k_triangulate) and vlgba_triangulate_ex
int triangulate_run(int m, const double *K, const double *T, const double *w, const double *kd,
                    long long n, const long long *obs_ptr, const int *obs_cam,
                    const double *obs_x, int device, double *X, int *status)
{
    if (int rc = check_tracks(m, K, T, w, n, obs_ptr, obs_cam, obs_x, X)) return rc;
    if (n == 0) return 0;
    if ((n + TRI_WAVE - 1) / TRI_WAVE > 0x7fffffffLL) return VLGBA_E_ARG;
    VLGBA_CHECK(hipSetDevice(device));
    rs_pool pool{device, nullptr, nullptr, 0};
    if (rs_acquire(device, 0, pool)) {
        if (pool.s) rs_release(pool);
        return -1;
    }
    hipStream_t s = pool.s;
    int rc = 0;
    {
        tri_dev d;
        double *d_X = nullptr;
        int *d_st = nullptr;
        const unsigned grid = (unsigned)((n + TRI_WAVE - 1) / TRI_WAVE);
        do {
            if ((rc = d.upload(m, K, T, w, n, obs_ptr, obs_cam, obs_x, s, kd)) ||
                (rc = dmalloc_n(&d_X, 4 * (size_t)n)) || (rc = dmalloc_n(&d_st, (size_t)n)))
                break;
            if (kd)
                k_triangulate_radial<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, d.kd,
                                                               d_X, d_st);
            else
                k_triangulate<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, d_X, d_st);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(X, d_X, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, s) !=
                    hipSuccess ||
                (status && hipMemcpyAsync(status, d_st, sizeof(int) * n, hipMemcpyDeviceToHost,
                                          s) != hipSuccess) ||
                hipStreamSynchronize(s) != hipSuccess)
                rc = -1;
        } while (0);
        (void)hipStreamSynchronize(s);
        if (d_X) ba_dfree(d_X);
        if (d_st) ba_dfree(d_st);
    }
    rs_release(pool);
    return rc;
}

// vlgba_intersect (md null: k_intersect_pass<false>) and vlgba_intersect_ex
// (k_intersect_pass<true> in every mode, then res_out / w_out at the returned X)
int intersect_run(int m, const double *K, const double *T, const double *w, long long n,
                  const long long *obs_ptr, const int *obs_cam, const double *obs_x,
                  const vlgba_options *opt, const isect_mode *md, double *X, double *error_out,
                  int error_cap, int *num_error, double *res_out, double *w_out,
                  vlgba_stats *stats)
{
    if (int rc = check_tracks(m, K, T, w, n, obs_ptr, obs_cam, obs_x, X)) return rc;
    if (error_out && error_cap < 0) return VLGBA_E_ARG;
    if (n == 0) return 0;
    if ((n + TRI_WAVE - 1) / TRI_WAVE > 0x7fffffffLL) return VLGBA_E_ARG;
    vlgba_options dflt;
    std::memset(&dflt, 0, sizeof dflt);
    if (!opt) opt = &dflt;
    VLGBA_CHECK(hipSetDevice(opt->device));
    const auto t0 = std::chrono::steady_clock::now();
    rs_pool pool{opt->device, nullptr, nullptr, 0};
    if (rs_acquire(opt->device, 6 * (size_t)n, pool)) {
        if (pool.s) rs_release(pool);
        return -1;
    }
    hipStream_t s = pool.s;
    double *h_lam = pool.pin, *h_fl = pool.pin + n, *h_out = pool.pin + 2 * (size_t)n;
    batch_lm lm((size_t)n, opt);   // the LM control, per point (ba_batch_lm.h)
    for (long long i = 0; i < n; i++)   // a point with no views is left untouched
        if (obs_ptr[i + 1] == obs_ptr[i]) lm.active[i] = 0;
    const long long N = obs_ptr[n];
    int rc = 0;
    {
        tri_dev d;
        double *d_b = nullptr, *d_bn = nullptr, *d_st = nullptr, *d_lam = nullptr,
               *d_out = nullptr, *d_res = nullptr;
        const unsigned grid = (unsigned)((n + TRI_WAVE - 1) / TRI_WAVE);
        do {
            if ((rc = d.upload(m, K, T, w, n, obs_ptr, obs_cam, obs_x, s, md ? md->kd : nullptr)) ||
                (rc = dmalloc_n(&d_b, 3 * (size_t)n)) || (rc = dmalloc_n(&d_bn, 3 * (size_t)n)) ||
                (rc = dmalloc_n(&d_st, (size_t)TRI_NST * n)) ||
                (rc = dmalloc_n(&d_lam, 2 * (size_t)n)) || (rc = dmalloc_n(&d_out, 4 * (size_t)n)))
                break;
            if (hipMemcpyAsync(d_b, X, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s) !=
                hipSuccess) {
                rc = -1;
                break;
            }
            isect_mode dm{nullptr, 0, 0, 0.0};
            if (md) {
                dm = *md;
                dm.kd = d.kd;   // the device copy
            }
            while (lm.stage(h_lam, h_fl)) {
                if (hipMemcpyAsync(d_lam, h_lam, sizeof(double) * 2 * n, hipMemcpyHostToDevice,
                                   s) != hipSuccess) {
                    rc = -1;
                    break;
                }
                if (md)
                    k_intersect_pass<true><<<grid, TRI_WAVE, 0, s>>>(
                        n, d.ptr, d.cam, d.x, d.rec, dm, d_b, d_bn, d_st, d_lam, d_lam + n, d_out);
                else
                    k_intersect_pass<false><<<grid, TRI_WAVE, 0, s>>>(
                        n, d.ptr, d.cam, d.x, d.rec, dm, d_b, d_bn, d_st, d_lam, d_lam + n, d_out);
                if (hipGetLastError() != hipSuccess ||
                    hipMemcpyAsync(h_out, d_out, sizeof(double) * 4 * n, hipMemcpyDeviceToHost,
                                   s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess) {
                    rc = -1;
                    break;
                }
                lm.apply(h_out, obs_ptr);
            }
            if (rc) break;
            // the last accepted step's parameters
            std::vector<double> bn(3 * (size_t)n);
            if (hipMemcpyAsync(X, d_b, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s) !=
                    hipSuccess ||
                hipMemcpyAsync(bn.data(), d_bn, sizeof(double) * 3 * n, hipMemcpyDeviceToHost,
                               s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess) {
                rc = -1;
                break;
            }
            for (long long i = 0; i < n; i++)
                if (lm.accepted_prev[i])
                    std::memcpy(X + 3 * i, bn.data() + 3 * i, sizeof(double) * 3);
            lm.write_errors(error_out, error_cap, num_error);
            if (md && N > 0 && (res_out || w_out)) {   // at the returned points
                if ((rc = dmalloc_n(&d_res, 3 * (size_t)N))) break;
                if (hipMemcpyAsync(d_b, X, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s) !=
                    hipSuccess) {
                    rc = -1;
                    break;
                }
                k_intersect_residuals<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, dm, d_b,
                                                                d_res, d_res + 2 * (size_t)N);
                if (hipGetLastError() != hipSuccess ||
                    (res_out && hipMemcpyAsync(res_out, d_res, sizeof(double) * 2 * N,
                                               hipMemcpyDeviceToHost, s) != hipSuccess) ||
                    (w_out && hipMemcpyAsync(w_out, d_res + 2 * (size_t)N, sizeof(double) * N,
                                             hipMemcpyDeviceToHost, s) != hipSuccess) ||
                    hipStreamSynchronize(s) != hipSuccess)
                    rc = -1;
            }
        } while (0);
        (void)hipStreamSynchronize(s);
        for (void *p : {(void *)d_b, (void *)d_bn, (void *)d_st, (void *)d_lam, (void *)d_out,
                        (void *)d_res})
            if (p) ba_dfree(p);
    }
    rs_release(pool);
    lm.fill_stats(stats, t0);
    return rc;
}
}   // namespace

extern "C" int vlgba_triangulate(int m, const double *K, const double *T, const double *w,
                                 long long n, const long long *obs_ptr, const int *obs_cam,
                                 const double *obs_x, int device, double *X, int *status)
{
    return triangulate_run(m, K, T, w, nullptr, n, obs_ptr, obs_cam, obs_x, device, X, status);
}

extern "C" int vlgba_triangulate_ex(int m, const double *K, const double *T, const double *w,
                                    const double *kd, long long n, const long long *obs_ptr,
                                    const int *obs_cam, const double *obs_x, int device, double *X,
                                    int *status)
{
    return triangulate_run(m, K, T, w, kd, n, obs_ptr, obs_cam, obs_x, device, X, status);
}

extern "C" int vlgba_intersect(int m, const double *K, const double *T, const double *w,
                               long long n, const long long *obs_ptr, const int *obs_cam,
                               const double *obs_x, const vlgba_options *opt, double *X,
                               double *error_out, int error_cap, int *num_error,
                               vlgba_stats *stats)
{
    return intersect_run(m, K, T, w, n, obs_ptr, obs_cam, obs_x, opt, nullptr, X, error_out,
                         error_cap, num_error, nullptr, nullptr, stats);
}

extern "C" int vlgba_intersect_ex(int m, const double *K, const double *T, const double *w,
                                  const double *kd, long long n, const long long *obs_ptr,
                                  const int *obs_cam, const double *obs_x,
                                  const vlgba_options *opt, int jacobian, int loss,
                                  double loss_scale, double *X, double *error_out, int error_cap,
                                  int *num_error, double *res_out, double *w_out,
                                  vlgba_stats *stats)
{
    if (int rc = batch_check_mode(jacobian, loss, loss_scale, kd != nullptr)) return rc;
    const isect_mode md{kd, jacobian, loss, loss != VLGBA_LOSS_NONE ? loss_scale : 0.0};
    return intersect_run(m, K, T, w, n, obs_ptr, obs_cam, obs_x, opt, &md, X, error_out,
                         error_cap, num_error, res_out, w_out, stats);
}

