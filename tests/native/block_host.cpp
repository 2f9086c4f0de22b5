// Host build of the batched one-block entries' shared code, for
// tests/test_block_host.py: the LM driver of csrc/ba_batch_lm.h on a CPU backend
// that calls the per-point pass of csrc/ba_triang_math.h, the triangulation of
// one point, the NA x NA solve of csrc/ba_small_solve.h, and the driver on a
// stub backend that reports a script.  No HIP header is needed to build it.
#include "../../bundleadjustmentmatlab_amd/csrc/ba_batch_lm.h"
#include "../../bundleadjustmentmatlab_amd/csrc/ba_small_solve.h"
#include "../../bundleadjustmentmatlab_amd/csrc/ba_triang_math.h"

namespace {
// the cameras' records, as k_tri_cameras forms them
std::vector<double> records(int m, const double *K, const double *T, const double *w, bool radial)
{
    std::vector<double> rec((size_t)TRI_CAM * m);
    for (int j = 0; j < m; j++) {
        const double k4[4] = {K[4 * j], K[4 * j + (radial ? 0 : 1)], K[4 * j + 2], K[4 * j + 3]};
        tri_camera(k4, T + 3 * j, w + 3 * j, rec.data() + (size_t)TRI_CAM * j);
    }
    return rec;
}

// the per-point pass over all points, one after the other
template <bool M>
struct host_points final : batch_backend {
    long long n;
    const long long *ptr;
    const int *cam;
    const double *x, *rec;
    isect_mode md;
    std::vector<double> b, bn, st;
    int pass(const double *lam, const double *flags, double *out) override
    {
        for (long long i = 0; i < n; i++)
            isect_pass_point<M>(i, n, ptr, cam, x, rec, &md, b.data(), bn.data(), st.data(),
                                (int)flags[i], lam[i], out);
        return 0;
    }
    int fetch(double *xo, double *xn) override
    {
        std::memcpy(xo, b.data(), sizeof(double) * b.size());
        std::memcpy(xn, bn.data(), sizeof(double) * bn.size());
        return 0;
    }
};

template <bool M>
int intersect(int m, const double *K, const double *T, const double *w, long long n,
              const long long *ptr, const int *cam, const double *x, const vlgba_options *opt,
              isect_mode md, double *X, double *err, int cap, int *nerr, vlgba_stats *stats)
{
    const std::vector<double> rec = records(m, K, T, w, md.kd != nullptr);
    host_points<M> be;
    be.n = n, be.ptr = ptr, be.cam = cam, be.x = x, be.rec = rec.data(), be.md = md;
    be.b.assign(X, X + 3 * n);
    be.bn.assign(3 * (size_t)n, 0.0);
    be.st.assign((size_t)TRI_NST * n, 0.0);
    batch_lm lm((size_t)n, opt);
    for (long long i = 0; i < n; i++)
        if (ptr[i + 1] == ptr[i]) lm.active[i] = 0;
    std::vector<double> stage(6 * (size_t)n);
    return batch_lm_run(lm, be, stage.data(), 3, ptr, X, err, cap, nerr, stats,
                        std::chrono::steady_clock::now());
}

// reports script[pass][problem][4] to every active problem
struct scripted final : batch_backend {
    size_t np;
    int npass, done = 0;
    const double *script;
    int pass(const double *, const double *flags, double *out) override
    {
        if (done >= npass) return -1;
        for (size_t q = 0; q < np; q++)
            if ((int)flags[q] & 1)
                std::memcpy(out + 4 * q, script + 4 * (np * done + q), sizeof(double) * 4);
        done++;
        return 0;
    }
    int fetch(double *x, double *xn) override
    {
        for (size_t q = 0; q < np; q++) x[q] = 0.0, xn[q] = 1.0;
        return 0;
    }
};
}   // namespace

// mode < 0: the pass without a mode (vlgba_intersect's); else vlgba_intersect_ex's
// with kd (or null), jac, loss, c
extern "C" int bh_intersect(int m, const double *K, const double *T, const double *w, long long n,
                            const long long *ptr, const int *cam, const double *x,
                            const vlgba_options *opt, int mode, const double *kd, int jac, int loss,
                            double c, double *X, double *err, int cap, int *nerr,
                            vlgba_stats *stats)
{
    if (mode < 0)
        return intersect<false>(m, K, T, w, n, ptr, cam, x, opt, isect_mode{nullptr, 0, 0, 0.0}, X,
                                err, cap, nerr, stats);
    return intersect<true>(m, K, T, w, n, ptr, cam, x, opt, isect_mode{kd, jac, loss, c}, X, err,
                           cap, nerr, stats);
}

// tri_point<false> (kd null) or tri_point<true> of every point: X (4 n), status
extern "C" void bh_triangulate(int m, const double *K, const double *T, const double *w,
                               const double *kd, long long n, const long long *ptr, const int *cam,
                               const double *x, double *X, int *status)
{
    const std::vector<double> rec = records(m, K, T, w, kd != nullptr);
    for (long long i = 0; i < n; i++) {
        const long long o = ptr[i], nv = ptr[i + 1] - o;
        status[i] = kd ? tri_point<true>(nv, cam + o, x + 2 * o, rec.data(), kd, X + 4 * i)
                       : tri_point<false>(nv, cam + o, x + 2 * o, rec.data(), kd, X + 4 * i);
    }
}

// the solve as the pass calls it: st = U | eA (column major), da out; returns
// the fallback flag, or -1 for an na without a kernel
extern "C" int bh_small_solve(int na, const double *st, double lambda, double *da)
{
    double S[100], rhs[10];
    switch (na) {
    case 6: return small_solve_damped<6>(st, lambda, S, rhs, da);
    case 7: return small_solve_damped<7>(st, lambda, S, rhs, da);
    case 9: return small_solve_damped<9>(st, lambda, S, rhs, da);
    case 10: return small_solve_damped<10>(st, lambda, S, rhs, da);
    default: return -1;
    }
}

// the driver over np problems of one parameter each on the scripted backend;
// x (np) ends as 1 for a problem whose last pass was accepted, else 0
extern "C" int bh_scripted(int np, const long long *ptr, const vlgba_options *opt, int npass,
                           const double *script, double *x, double *err, int cap, int *nerr,
                           vlgba_stats *stats)
{
    scripted be;
    be.np = (size_t)np, be.npass = npass, be.script = script;
    batch_lm lm((size_t)np, opt);
    std::vector<double> stage(6 * (size_t)np);
    return batch_lm_run(lm, be, stage.data(), 1, ptr, x, err, cap, nerr, stats,
                        std::chrono::steady_clock::now());
}
