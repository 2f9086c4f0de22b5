// ba_batch_dev.cpp -- the per-device pool of streams and pinned blocks and the
// device backend of the batched one-block LM (ba_batch_dev.h).  Host code only.
#include "ba_batch_dev.h"

#include <mutex>

namespace {
struct pooled {
    int device;
    hipStream_t s;
    double *pin;
    size_t cap;   // doubles
};
std::mutex g_pool_mu;
std::vector<pooled> g_pool;

struct batch_dev final : batch_backend {
    hipStream_t s;
    size_t np, nx;
    const batch_dev_fn &launch;
    ba_dbuf<double> x, xn, lam, out;   // lam: lam | flags
    batch_dev(hipStream_t s_, size_t np_, size_t nx_, const batch_dev_fn &l)
        : s(s_), np(np_), nx(nx_), launch(l)
    {
    }
    ~batch_dev() override { (void)hipStreamSynchronize(s); }   // before the buffers go
    batch_dev_io io() const { return {x, xn, lam, lam + np, out}; }
    int pass(const double *h_lam, const double *, double *h_out) override
    {
        TRY_RC(upload(lam.get(), h_lam, 2 * np, s));   // flags == lam + np
        TRY_RC(launch(io()));
        VLGBA_CHECK(hipGetLastError());
        TRY_RC(download(h_out, out.get(), 4 * np, s));
        VLGBA_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    int fetch(double *h_x, double *h_xn) override
    {
        TRY_RC(download(h_x, x.get(), nx * np, s));
        TRY_RC(download(h_xn, xn.get(), nx * np, s));
        VLGBA_CHECK(hipStreamSynchronize(s));
        return 0;
    }
};
}   // namespace

batch_stream::batch_stream(int device, size_t need) : rc(0), device_(device)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t q = 0; q < g_pool.size(); q++)
            if (g_pool[q].device == device) {
                s = g_pool[q].s;
                pin = g_pool[q].pin;
                cap_ = g_pool[q].cap;
                g_pool.erase(g_pool.begin() + (long)q);
                break;
            }
    }
    if (!s) rc = -(int)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (!rc && cap_ < need) {
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        cap_ = 0;
        const size_t cap = need > 4096 ? need : 4096;
        rc = -(int)hipHostMalloc((void **)&pin, sizeof(double) * cap, hipHostMallocDefault);
        if (!rc) cap_ = cap;
    }
}

batch_stream::~batch_stream()
{
    if (!s) return;
    (void)hipStreamSynchronize(s);
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool.push_back(pooled{device_, s, pin, cap_});
}

int batch_dev_run(batch_stream &bs, batch_lm &lm, int nx, const long long *obs_ptr, double *x,
                  double *error_out, int error_cap, int *num_error, vlgba_stats *stats,
                  std::chrono::steady_clock::time_point t0, const batch_dev_fn &pass,
                  const batch_dev_fn &residuals)
{
    batch_dev be(bs.s, lm.np, (size_t)nx, pass);
    TRY_RC(be.x.alloc(be.nx * be.np));
    TRY_RC(be.xn.alloc(be.nx * be.np));
    TRY_RC(be.lam.alloc(2 * be.np));
    TRY_RC(be.out.alloc(4 * be.np));
    TRY_RC(upload(be.x.get(), x, be.nx * be.np, bs.s));
    TRY_RC(batch_lm_run(lm, be, bs.pin, nx, obs_ptr, x, error_out, error_cap, num_error, stats,
                        t0));
    if (!residuals) return 0;
    TRY_RC(upload(be.x.get(), x, be.nx * be.np, bs.s));   // at the returned parameters
    TRY_RC(residuals(be.io()));
    VLGBA_CHECK(hipStreamSynchronize(bs.s));
    return 0;
}
