// ba_mex.cpp -- the MEX-compatible stage entries (vlgba_mex_bundle*: the
// reference's three MEX files on dense m x n layouts, one stage-mode context
// per call) and vlgba_debug_pinv_solve.  Host code only.
//
// Host buffers that a queued copy reads or writes are declared before the
// context's owner, so the owner (which synchronises the streams) goes first on
// every path.
#include "ba_ctx.h"

#include <dlfcn.h>

#include <cstring>

namespace {

void obs_from_vis(int m, int n, const double *vis, std::vector<int> &pt, std::vector<int> &cam)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++)
            if (vis[i + (size_t)n * j] != 0.0) {
                pt.push_back(i);
                cam.push_back(j);
            }
}

// a stage-mode context for the observations (pt, cam, ox)
int mex_ctx(int model, int m, int n, int num_a, const std::vector<int> &pt,
            const std::vector<int> &cam, const std::vector<double> &ox, const double *K,
            bool lower_blocks, ctx_ptr &out)
{
    const vlgba_problem pr = {m, n, num_a, (long long)pt.size(), pt.data(), cam.data(), ox.data(),
                              K, 0.0, model};
    vlgba_ctx *c = nullptr;
    TRY_RC(ctx_create(&pr, nullptr, &c, lower_blocks, true, true));
    out.reset(c);
    return 0;
}

// stage 1 on the device: the records (A | e), W, the projections and B per
// observation, U / eA / V / eB straight into the caller's arrays
int mex1_device(vlgba_ctx *c, const double *a, const double *b, std::vector<double> &jr,
                std::vector<double> &hW, std::vector<double> &xh, std::vector<double> &hB,
                double *U, double *V, double *eA, double *eB)
{
    ba_dev &d = c->d;
    const size_t N = (size_t)d.N, na = (size_t)d.na;
    jr.resize((size_t)d.js * N);
    hW.resize(3 * na * N);
    xh.resize(2 * N);
    hB.resize(6 * N);
    TRY_RC(ctx_alloc(c, &d.xh_out, 2 * N));
    TRY_RC(ctx_alloc(c, &d.B_out, 6 * N));
    TRY_RC(upload(d.a, a, (size_t)d.ld, d.stream));
    TRY_RC(upload(d.b, b, 3 * (size_t)d.n, d.stream));
    const ba_flags f = {0, 0, 0};
    TRY_RC(ba_launch_rotations(&d, d.a, d.rot));
    TRY_RC(ba_launch_linearize(&d, f));
    TRY_RC(ba_launch_camera_reduce(&d, f, d.stream));
    TRY_RC(download(jr.data(), d.jrec, jr.size(), d.stream));
    TRY_RC(download(hW.data(), d.W, hW.size(), d.stream));
    TRY_RC(download(xh.data(), d.xh_out, xh.size(), d.stream));
    TRY_RC(download(hB.data(), d.B_out, hB.size(), d.stream));
    TRY_RC(download(U, d.U, na * na * d.m, d.stream));
    TRY_RC(download(eA, d.eA, na * d.m, d.stream));
    TRY_RC(download(V, d.V, 9 * (size_t)d.n, d.stream));
    TRY_RC(download(eB, d.eB, 3 * (size_t)d.n, d.stream));
    return hipStreamSynchronize(d.stream) == hipSuccess ? 0 : -1;
}

int mex1_impl(int model, int m, int n, int num_a, const double *K, const double *a,
              const double *b, const double *X, const double *vis, double *X_hat, double *A,
              double *B, double *e, double *U, double *V, double *W, double *eA, double *eB)
{
    if (m < 1 || n < 0 || (!K && model == VLGBA_MODEL_EUCLIDEAN) || !a || !b || !X || !vis)
        return VLGBA_E_ARG;
    std::vector<int> pt, cam;
    obs_from_vis(m, n, vis, pt, cam);
    const long long N = (long long)pt.size();
    std::vector<double> ox(2 * N);
    for (long long q = 0; q < N; q++) {
        const size_t p = (size_t)pt[q] + (size_t)n * cam[q];
        ox[2 * q] = X[2 * p];
        ox[2 * q + 1] = X[2 * p + 1];
    }
    std::vector<double> jr, hW, xh, hB;
    {
        ctx_ptr c;
        TRY_RC(mex_ctx(model, m, n, num_a, pt, cam, ox, K, true, c));
        TRY_RC(mex1_device(c.get(), a, b, jr, hW, xh, hB, U, V, eA, eB));
    }
    // scatter to the dense MEX layouts; invisible pairs: X_hat = X, zeros
    const size_t nm = (size_t)n * m;
    for (size_t p = 0; p < nm; p++) {
        X_hat[2 * p] = X[2 * p];
        X_hat[2 * p + 1] = X[2 * p + 1];
        e[2 * p] = e[2 * p + 1] = 0.0;
    }
    std::memset(A, 0, sizeof(double) * 2 * num_a * nm);
    std::memset(B, 0, sizeof(double) * 6 * nm);
    std::memset(W, 0, sizeof(double) * 3 * num_a * nm);
    const int js = 2 * num_a + 2;
    for (long long q = 0; q < N; q++) {
        const size_t p = (size_t)pt[q] + (size_t)n * cam[q];
        X_hat[2 * p] = xh[2 * q];
        X_hat[2 * p + 1] = xh[2 * q + 1];
        std::memcpy(A + 2 * num_a * p, jr.data() + js * q, sizeof(double) * 2 * num_a);
        e[2 * p] = jr[js * q + 2 * num_a];
        e[2 * p + 1] = jr[js * q + 2 * num_a + 1];
        std::memcpy(B + 6 * p, hB.data() + 6 * q, sizeof(double) * 6);
        std::memcpy(W + 3 * num_a * p, hW.data() + 3 * num_a * q, sizeof(double) * 3 * num_a);
    }
    return 0;
}

int mex2_impl(int model, int m, int n, int num_a, const double *Y, const double *W,
              const double *U, const double *eA, const double *eB, double *S, double *e_)
{
    if (m < 1 || n < 0 || !Y || !W || !U || !eA || !eB || !S || !e_) return VLGBA_E_ARG;
    const int bs = 3 * num_a;
    std::vector<int> pt, cam;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) {
            const size_t p = (size_t)i + (size_t)n * j;
            bool nz = false;
            for (int q = 0; q < bs && !nz; q++) nz = (Y[bs * p + q] != 0.0) || (W[bs * p + q] != 0.0);
            if (nz) {
                pt.push_back(i);
                cam.push_back(j);
            }
        }
    const long long N = (long long)pt.size();
    std::vector<double> ox(2 * N, 0.0), hY((size_t)bs * N), hW((size_t)bs * N);
    for (long long q = 0; q < N; q++) {
        const size_t p = (size_t)pt[q] + (size_t)n * cam[q];
        std::memcpy(hY.data() + bs * q, Y + bs * p, sizeof(double) * bs);
        std::memcpy(hW.data() + bs * q, W + bs * p, sizeof(double) * bs);
    }
    const std::vector<double> K(4 * (size_t)m, 1.0);
    ctx_ptr c;
    TRY_RC(mex_ctx(model, m, n, num_a, pt, cam, ox, K.data(), false, c));
    ba_dev &d = c->d;
    const long long ld = d.ld;
    double *Sd = nullptr;
    TRY_RC(ctx_alloc(c.get(), &Sd, (size_t)(ld * ld)));
    TRY_RC(upload(d.Y, hY.data(), hY.size(), d.stream));
    TRY_RC(upload(d.W, hW.data(), hW.size(), d.stream));
    TRY_RC(upload(d.U, U, (size_t)num_a * num_a * m, d.stream));
    TRY_RC(upload(d.eA, eA, (size_t)num_a * m, d.stream));
    TRY_RC(upload(d.eB, eB, 3 * (size_t)n, d.stream));
    TRY_RC(ba_launch_yeb(&d));
    // U is given already damped (bundle_euclid.m:192 passes U_): lambda = 0
    TRY_RC(ba_launch_schur(&d, 0.0));
    TRY_RC(ba_launch_assemble_plain(&d, Sd, ld, 0));
    TRY_RC(download(S, Sd, (size_t)(ld * ld), d.stream));
    TRY_RC(download(e_, d.rhs, (size_t)ld, d.stream));
    return hipStreamSynchronize(d.stream) == hipSuccess ? 0 : -1;
}

int mex3_impl(int model, int m, int n, int num_a, const double *W, const double *da,
              const double *eB, const double *Vinv, const double *K, const double *a,
              const double *b, const double *X, const double *vis, double *db, double *a_new,
              double *b_new, double *X_hat)
{
    if (m < 1 || n < 0 || !W || !da || !eB || !Vinv ||
        (!K && model == VLGBA_MODEL_EUCLIDEAN) || !a || !b || !X || !vis)
        return VLGBA_E_ARG;
    const int bs = 3 * num_a;
    std::vector<int> pt, cam;
    std::vector<unsigned char> ov;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) {
            const size_t p = (size_t)i + (size_t)n * j;
            bool nz = vis[p] != 0.0;
            const bool v = nz;
            for (int q = 0; q < bs && !nz; q++) nz = W[bs * p + q] != 0.0;
            if (nz) {
                pt.push_back(i);
                cam.push_back(j);
                ov.push_back(v ? 1 : 0);
            }
        }
    const long long N = (long long)pt.size();
    std::vector<double> ox(2 * N), hW((size_t)bs * N), xh(2 * N);
    for (long long q = 0; q < N; q++) {
        const size_t p = (size_t)pt[q] + (size_t)n * cam[q];
        ox[2 * q] = X[2 * p];
        ox[2 * q + 1] = X[2 * p + 1];
        std::memcpy(hW.data() + bs * q, W + bs * p, sizeof(double) * bs);
    }
    {
        ctx_ptr c;
        TRY_RC(mex_ctx(model, m, n, num_a, pt, cam, ox, K, true, c));
        ba_dev &d = c->d;
        TRY_RC(ctx_alloc(c.get(), &d.xh_out, 2 * (size_t)N));
        TRY_RC(ctx_alloc(c.get(), &d.obs_vis, (size_t)N));
        TRY_RC(upload(d.obs_vis, ov.data(), ov.size(), d.stream));
        TRY_RC(upload(d.W, hW.data(), hW.size(), d.stream));
        TRY_RC(upload(d.da, da, (size_t)d.ld, d.stream));
        TRY_RC(upload(d.eB, eB, 3 * (size_t)n, d.stream));
        TRY_RC(upload(d.Vinv, Vinv, 9 * (size_t)n, d.stream));
        TRY_RC(upload(d.a, a, (size_t)d.ld, d.stream));
        TRY_RC(upload(d.b, b, 3 * (size_t)n, d.stream));
        VLGBA_CHECK(hipMemsetAsync(d.eA, 0, sizeof(double) * d.ld, d.stream));
        TRY_RC(ba_launch_update(&d, 0.0, ba_flags{}, false, false, nullptr));
        TRY_RC(download(db, d.db, 3 * (size_t)n, d.stream));
        TRY_RC(download(a_new, d.a_new, (size_t)d.ld, d.stream));
        TRY_RC(download(b_new, d.b_new, 3 * (size_t)n, d.stream));
        TRY_RC(download(xh.data(), d.xh_out, xh.size(), d.stream));
        if (hipStreamSynchronize(d.stream) != hipSuccess) return -1;
    }
    const size_t nm = (size_t)n * m;
    for (size_t p = 0; p < nm; p++) {
        X_hat[2 * p] = X[2 * p];
        X_hat[2 * p + 1] = X[2 * p + 1];
    }
    for (long long q = 0; q < N; q++) {
        if (!ov[q]) continue;
        const size_t p = (size_t)pt[q] + (size_t)n * cam[q];
        X_hat[2 * p] = xh[2 * q];
        X_hat[2 * p + 1] = xh[2 * q + 1];
    }
    return 0;
}

// a rocBLAS handle of vlgba_debug_pinv_solve's own.  Declared after the device
// buffers its work uses: the device is idle and the handle gone before they are
// freed, on every path.
struct own_handle {
    rocblas_handle h = nullptr;
    ~own_handle()
    {
        (void)hipDeviceSynchronize();
        if (!h) return;
        auto destroy =
            (rocblas_status(*)(rocblas_handle))dlsym(RTLD_DEFAULT, "rocblas_destroy_handle");
        if (destroy) destroy(h);
    }
};

}   // namespace

extern "C" {

int vlgba_debug_pinv_solve(int ld, const double *S, const double *e_, double *da)
{
    if (ld < 1 || !S || !e_ || !da) return VLGBA_E_ARG;
    rs_api *rs = rs_load();
    if (!rs) return VLGBA_E_ARG;
    int dev = 0;
    VLGBA_CHECK(hipGetDevice(&dev));
    ba_dev d;
    std::memset(&d, 0, sizeof d);
    d.device = dev;
    d.stream = nullptr;   // legacy stream: synchronous below
    const size_t n = (size_t)ld;
    ba_dbuf<double> buf;
    ba_dbuf<int> info;
    TRY_RC(buf.alloc(n * n + 4 * n));
    TRY_RC(info.alloc(1));
    own_handle hdl;
    double *A = buf, *ev = A + n * n, *e = ev + n, *w = e + n, *rhs = w + n;
    if (hipMemcpy(A, S, sizeof(double) * n * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rhs, e_, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess)
        return -1;
    if (rs->create(&hdl.h) != rocblas_status_success ||
        rs->syevd(hdl.h, rocblas_evect_original, rocblas_fill_lower, ld, A, ld, ev, e, info) !=
            rocblas_status_success)
        return VLGBA_E_ARG;
    TRY_RC(ba_pinv_apply(&d, A, ev, ld, rhs, w, e));
    return hipMemcpy(da, e, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

int vlgba_mex_bundle_1(int m, int n, int num_a, const double *K, const double *a,
                       const double *b, const double *X, const double *vis, double *X_hat,
                       double *A, double *B, double *e, double *U, double *V, double *W,
                       double *eA, double *eB)
{
    if (num_a == BA_PROJ_NA) return VLGBA_E_NUMA;   // the projective stage has its own entry
    return mex1_impl(VLGBA_MODEL_EUCLIDEAN, m, n, num_a, K, a, b, X, vis, X_hat, A, B, e, U, V,
                     W, eA, eB);
}

int vlgba_mex_bundle_2(int m, int n, int num_a, const double *Y, const double *W,
                       const double *U, const double *eA, const double *eB, double *S,
                       double *e_)
{
    // mex_bundle_2_Se_.c reads num_a = rows(Y) (:57); 12 is the projective twin's
    return mex2_impl(num_a == BA_PROJ_NA ? VLGBA_MODEL_PROJECTIVE : VLGBA_MODEL_EUCLIDEAN, m, n,
                     num_a, Y, W, U, eA, eB, S, e_);
}

int vlgba_mex_bundle_3(int m, int n, int num_a, const double *W, const double *da,
                       const double *eB, const double *Vinv, const double *K, const double *a,
                       const double *b, const double *X, const double *vis, double *db,
                       double *a_new, double *b_new, double *X_hat)
{
    if (num_a == BA_PROJ_NA) return VLGBA_E_NUMA;
    return mex3_impl(VLGBA_MODEL_EUCLIDEAN, m, n, num_a, W, da, eB, Vinv, K, a, b, X, vis, db,
                     a_new, b_new, X_hat);
}

int vlgba_mex_bundle_proj_1(int m, int n, const double *a, const double *b, const double *X,
                            const double *vis, double *X_hat, double *A, double *B, double *e,
                            double *U, double *V, double *W, double *eA, double *eB)
{
    return mex1_impl(VLGBA_MODEL_PROJECTIVE, m, n, BA_PROJ_NA, nullptr, a, b, X, vis, X_hat, A,
                     B, e, U, V, W, eA, eB);
}

int vlgba_mex_bundle_proj_2(int m, int n, const double *Y, const double *W, const double *U,
                            const double *eA, const double *eB, double *S, double *e_)
{
    return mex2_impl(VLGBA_MODEL_PROJECTIVE, m, n, BA_PROJ_NA, Y, W, U, eA, eB, S, e_);
}

int vlgba_mex_bundle_proj_3(int m, int n, const double *W, const double *da, const double *eB,
                            const double *Vinv, const double *a, const double *b,
                            const double *X, const double *vis, double *db, double *a_new,
                            double *b_new, double *X_hat)
{
    return mex3_impl(VLGBA_MODEL_PROJECTIVE, m, n, BA_PROJ_NA, W, da, eB, Vinv, nullptr, a, b, X,
                     vis, db, a_new, b_new, X_hat);
}

}   // extern "C"
