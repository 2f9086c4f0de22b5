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
// (host and device); the working set of a lane stays in registers.  The LM
// control is the driver of ba_batch_lm.h on the device backend of
// ba_batch_dev.h, as in ba_resect.hip: intersect_run checks the arguments,
// uploads the tracks and hands over a launch and a residual lambda.
//
// vlgba_triangulate_ex / vlgba_intersect_ex (include/vlgba.h) add the radial
// lens (k1, k2 per camera in a side array next to the unchanged records; the
// undistortion before triangulation.m's rows), the closed-form B and the robust
// losses: k_triangulate<true>, and k_intersect_pass<true>, beside the plain
// entries' <false>, in which the mode folds away.
#include "ba_batch_dev.h"
#include "ba_triang_math.h"

#include <cstring>

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

// RADIAL = false: vlgba_triangulate's kernel (kd is not read); true: radial
// lenses, every measurement undistorted first (tri_point<true>)
template <bool RADIAL>
__global__ __launch_bounds__(TRI_WAVE) void k_triangulate(
    long long n, const long long *__restrict__ obs_ptr, const int *__restrict__ obs_cam,
    const double *__restrict__ obs_x, const double *__restrict__ rec,
    const double *__restrict__ kd, double *__restrict__ X, int *__restrict__ status)
{
    const long long i = (long long)blockIdx.x * TRI_WAVE + threadIdx.x;
    if (i >= n) return;
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    double x[4];
    const int st = tri_point<RADIAL>(nv, obs_cam + o0, obs_x + 2 * o0, rec, kd, x);
    X[4 * i] = x[0];
    X[4 * i + 1] = x[1];
    X[4 * i + 2] = x[2];
    X[4 * i + 3] = x[3];
    status[i] = st;
}

// One lane per point runs isect_pass_point (ba_triang_math.h).  M = false:
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
    // staged with lambda as doubles (one copy a pass); vector loads at device
    // scope, as every per-pass word (ba_internal.h)
    const int fl = (int)__hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!(fl & 1)) return;                          // point finished (or without views)
    const double lambda = __hip_atomic_load(lam_p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    isect_pass_point<M>(i, n, obs_ptr, obs_cam, obs_x, rec, &md, b, b_new, state, fl, lambda, out);
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
    ba_dbuf<long long> ptr;
    ba_dbuf<int> cam;
    ba_dbuf<double> x, in, rec;
    double *kd = nullptr;   // k1, k2 per camera (in + 10 m) or null: pinhole
    int load(int m, const double *K, const double *T, const double *w, long long n,
             const long long *obs_ptr, const int *obs_cam, const double *obs_x, hipStream_t s,
             const double *kd_host)
    {
        const size_t N = (size_t)obs_ptr[n], M = (size_t)m;
        TRY_RC(ptr.alloc((size_t)n + 1));
        TRY_RC(cam.alloc(N));
        TRY_RC(x.alloc(2 * N));
        TRY_RC(in.alloc(12 * M));
        TRY_RC(rec.alloc(TRI_CAM * M));
        TRY_RC(upload(ptr.get(), obs_ptr, (size_t)n + 1, s));
        TRY_RC(upload(cam.get(), obs_cam, N, s));
        TRY_RC(upload(x.get(), obs_x, 2 * N, s));
        TRY_RC(upload(in.get(), K, 4 * M, s));
        TRY_RC(upload(in + 4 * M, T, 3 * M, s));
        TRY_RC(upload(in + 7 * M, w, 3 * M, s));
        if (kd_host) {
            kd = in + 10 * M;
            TRY_RC(upload(kd, kd_host, 2 * M, s));
        }
        k_tri_cameras<<<(m + TRI_WAVE - 1) / TRI_WAVE, TRI_WAVE, 0, s>>>(
            m, in, in + 4 * M, in + 7 * M, kd_host != nullptr, rec);
        return -(int)hipGetLastError();
    }
};

// vlgba_triangulate (kd null: k_triangulate<false>) and vlgba_triangulate_ex
int triangulate_run(int m, const double *K, const double *T, const double *w, const double *kd,
                    long long n, const long long *obs_ptr, const int *obs_cam,
                    const double *obs_x, int device, double *X, int *status)
{
    if (int rc = check_tracks(m, K, T, w, n, obs_ptr, obs_cam, obs_x, X)) return rc;
    if (n == 0) return 0;
    if ((n + TRI_WAVE - 1) / TRI_WAVE > 0x7fffffffLL) return VLGBA_E_ARG;
    VLGBA_CHECK(hipSetDevice(device));
    // before the stream's guard: freed after it has drained (ba_batch_dev.h)
    tri_dev d;
    ba_dbuf<double> d_X;
    ba_dbuf<int> d_st;
    batch_stream bs(device, 0);
    if (bs.rc) return bs.rc;
    hipStream_t s = bs.s;
    const unsigned grid = (unsigned)((n + TRI_WAVE - 1) / TRI_WAVE);
    TRY_RC(d.load(m, K, T, w, n, obs_ptr, obs_cam, obs_x, s, kd));
    TRY_RC(d_X.alloc(4 * (size_t)n));
    TRY_RC(d_st.alloc((size_t)n));
    const auto kern = kd ? k_triangulate<true> : k_triangulate<false>;
    kern<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, d.kd, d_X, d_st);
    VLGBA_CHECK(hipGetLastError());
    TRY_RC(download(X, d_X.get(), 4 * (size_t)n, s));
    if (status) TRY_RC(download(status, d_st.get(), (size_t)n, s));
    VLGBA_CHECK(hipStreamSynchronize(s));
    return 0;
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
    // before the stream's guard: freed after it has drained (ba_batch_dev.h)
    tri_dev d;
    ba_dbuf<double> d_st, d_res;
    batch_stream bs(opt->device, 6 * (size_t)n);
    if (bs.rc) return bs.rc;
    hipStream_t s = bs.s;
    batch_lm lm((size_t)n, opt);   // the LM control, per point (ba_batch_lm.h)
    for (long long i = 0; i < n; i++)   // a point with no views is left untouched
        if (obs_ptr[i + 1] == obs_ptr[i]) lm.active[i] = 0;
    const size_t N = (size_t)obs_ptr[n];
    const unsigned grid = (unsigned)((n + TRI_WAVE - 1) / TRI_WAVE);
    TRY_RC(d.load(m, K, T, w, n, obs_ptr, obs_cam, obs_x, s, md ? md->kd : nullptr));
    TRY_RC(d_st.alloc((size_t)TRI_NST * n));
    isect_mode dm{nullptr, 0, 0, 0.0};
    if (md) {
        dm = *md;
        dm.kd = d.kd;   // the device copy
    }
    const auto kern = md ? k_intersect_pass<true> : k_intersect_pass<false>;
    const batch_dev_fn pass = [&](const batch_dev_io &p) {
        kern<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, dm, p.x, p.x_new, d_st, p.lam,
                                       p.flags, p.out);
        return 0;
    };
    batch_dev_fn residuals;
    if (md && N > 0 && (res_out || w_out))
        residuals = [&](const batch_dev_io &p) {
            TRY_RC(d_res.alloc(3 * N));
            k_intersect_residuals<<<grid, TRI_WAVE, 0, s>>>(n, d.ptr, d.cam, d.x, d.rec, dm, p.x,
                                                            d_res, d_res + 2 * N);
            VLGBA_CHECK(hipGetLastError());
            if (res_out) TRY_RC(download(res_out, d_res.get(), 2 * N, s));
            if (w_out) TRY_RC(download(w_out, d_res + 2 * N, N, s));
            return 0;
        };
    return batch_dev_run(bs, lm, 3, obs_ptr, X, error_out, error_cap, num_error, stats, t0, pass,
                         residuals);
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
