// ba_cov_host.cpp -- the host driver of vlgba_covariance (kernels: ba_cov.hip,
// the selected inverse: ba_chol.hip) and its C ABI.  Its state is the
// context's ba_cov_state (ba_ctx.h).  Host code only.
#include "ba_ctx.h"
#include "ba_chol.h"   // the selected method reads the reduced solve's plan

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>

namespace {

// the context's covariance state, made on first use (null: out of memory)
ba_cov_state *cov_state(vlgba_ctx *c)
{
    if (!c->cov) c->cov.reset(new (std::nothrow) ba_cov_state());
    return c->cov.get();
}

// the co-visible blocks (j >= k) by camera row j, columns ascending: the CSR
// k_point_cov reads and the packed copy of Sigma_a's blocks
int cov_setup_blocks(vlgba_ctx *c, ba_cov_state &s)
{
    ba_dev &d = c->d;
    std::vector<int> jk(2 * (size_t)d.nb);
    TRY_RC(download(jk.data(), d.blk_jk, jk.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    std::vector<int> &ord = s.ord;
    ord.resize((size_t)d.nb);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int x, int y) {
        return jk[2 * (size_t)x] != jk[2 * (size_t)y] ? jk[2 * (size_t)x] < jk[2 * (size_t)y]
                                                      : jk[2 * (size_t)x + 1] < jk[2 * (size_t)y + 1];
    });
    std::vector<int> rowptr((size_t)d.m + 1, 0), col((size_t)d.nb), bj((size_t)d.nb);
    for (int p = 0; p < d.nb; p++) {
        bj[p] = jk[2 * (size_t)ord[p]];
        col[p] = jk[2 * (size_t)ord[p] + 1];
        if (bj[p] < 0 || bj[p] >= d.m || col[p] < 0 || col[p] > bj[p]) return VLGBA_E_ARG;
        rowptr[(size_t)bj[p] + 1]++;
    }
    for (int j = 0; j < d.m; j++) rowptr[(size_t)j + 1] += rowptr[j];
    TRY_RC(s.rowptr.alloc(rowptr.size()));
    TRY_RC(s.col.alloc(col.size()));
    TRY_RC(s.bj.alloc(bj.size()));
    TRY_RC(upload(s.rowptr.get(), rowptr.data(), rowptr.size(), d.stream));
    TRY_RC(upload(s.col.get(), col.data(), col.size(), d.stream));
    TRY_RC(upload(s.bj.get(), bj.data(), bj.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    // one block more than nb: the bisection of an empty row ends there
    const size_t cnt = ((size_t)d.nb + 1) * d.na * d.na;
    TRY_RC(s.packed.alloc(cnt));
    VLGBA_CHECK(hipMemsetAsync(s.packed, 0, sizeof(double) * cnt, d.stream));
    return 0;
}

// vlgba_covariance's per-context setup: the points binned by track length
// (ba_cov.hip) and the device buffers of its results
int cov_setup(vlgba_ctx *c, ba_cov_state &s)
{
    ba_dev &d = c->d;
    if (s.pts) return 0;
    std::vector<int> ptr((size_t)d.n + 1);
    TRY_RC(download(ptr.data(), d.pt_ptr, (size_t)d.n + 1, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    std::vector<int> bin[3];
    int tmax = 0, seen = 0;
    for (int i = 0; i < d.n; i++) {
        const int t = ptr[i + 1] - ptr[i];
        bin[t <= BA_COV_T8 ? 0 : t <= BA_COV_T64 ? 1 : 2].push_back(i);
        tmax = std::max(tmax, t);
        seen += t > 0;
    }
    std::vector<int> list;
    list.reserve((size_t)d.n);
    for (const auto &b : bin) list.insert(list.end(), b.begin(), b.end());
    TRY_RC(s.list.alloc(list.size()));
    TRY_RC(upload(s.list.get(), list.data(), list.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));   // list goes out of scope
    // VLGBA_COV_PACKED=0: the dense method's k_point_cov reads the dense inverse
    // (A/B); the packed copy is still filled, after the point kernel, for
    // vlgba_get_covariance_blocks
    const char *pk = std::getenv("VLGBA_COV_PACKED");
    s.src_packed = !(pk && pk[0] == '0');
    TRY_RC(cov_setup_blocks(c, s));
    TRY_RC(s.fixed.alloc((size_t)std::max(1LL, d.ld)));
    TRY_RC(s.diag.alloc((size_t)d.na * d.na * d.m));
    s.n8 = (int)bin[0].size();
    s.n64 = (int)bin[1].size();
    s.nwg = (int)bin[2].size();
    s.tmax = tmax;
    s.seen = seen;
    TRY_RC(s.pts.alloc(9 * (size_t)d.n));
    return 0;
}

// ... and of the selected method: the tile sources of its descent and its tiles
int cov_setup_selected(vlgba_ctx *c, ba_cov_state &s)
{
    ba_dev &d = c->d;
    if (s.sig) return 0;
    const int nt32 = d.chol->plan.nt32;   // (the selected method: a solving context)
    std::vector<int> src(2 * (size_t)nt32);
    TRY_RC(ba_cr32_selinv_sources(&d, src.data()));
    TRY_RC(s.selsrc.alloc(src.size()));
    TRY_RC(upload(s.selsrc.get(), src.data(), src.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));   // src goes out of scope
    const size_t cnt = (size_t)3 * 32 * 32 * nt32;
    ba_dbuf<double> sig;
    TRY_RC(sig.alloc(cnt));
    VLGBA_CHECK(hipMemsetAsync(sig, 0, sizeof(double) * cnt, d.stream));
    s.sig = std::move(sig);
    return 0;
}

// the three events that time a call's camera and point parts
struct cov_events {
    hipEvent_t ev[3] = {};
    int create()
    {
        for (auto &e : ev) VLGBA_CHECK(hipEventCreate(&e));
        return 0;
    }
    ~cov_events()
    {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

int cov_points(vlgba_ctx *c, const ba_cov_state &s, const ba_cov_src &src)
{
    return ba_launch_point_cov(&c->d, s.list, s.n8, s.n64, s.nwg, s.tmax, &src, s.pts);
}

// the selected method: S0 in the CR's tiles as a pass assembles it (unit
// diagonal on the exactly-zero rows), the fixed rows from the blocks, the
// per-level factor launches, the descent, and the co-visible blocks out of
// its tiles; no back substitution, da and the dense scratch untouched
int cov_run_selected(vlgba_ctx *c, ba_cov_state &s, const hipEvent_t ev[3])
{
    ba_dev &d = c->d;
    VLGBA_CHECK(hipEventRecord(ev[0], d.stream));
    TRY_RC(schur_phase(c, 0.0));
    TRY_RC(ba_launch_assemble(&d));
    TRY_RC(ba_cov_mark_fixed_blocks(&d, s.fixed));
    TRY_RC(ba_cr32_factor(&d));
    TRY_RC(ba_cr32_selinv(&d, s.selsrc, s.sig));
    TRY_RC(ba_cov_extract(&d, s.sig, s.fixed, s.bj, s.col, d.nb, s.diag, s.packed));
    VLGBA_CHECK(hipEventRecord(ev[1], d.stream));
    TRY_RC(cov_points(c, s, ba_cov_src{nullptr, d.ld, s.rowptr, s.col, s.packed}));
    VLGBA_CHECK(hipEventRecord(ev[2], d.stream));
    double pivot = 0.0;   // the CR's status word: a non-positive pivot
    TRY_RC(download(&pivot, d.scal + 4, 1, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return pivot != 0.0 ? VLGBA_E_SINGULAR : 0;
}

// the dense method: dpotrf / dpotri on the dense scratch
int cov_run_dense(vlgba_ctx *c, ba_cov_state &s, rs_api *rs, rocblas_handle hdl,
                  const hipEvent_t ev[3])
{
    ba_dev &d = c->d;
    const long long ld = d.ld;
    double *S = c->dense.S;
    VLGBA_CHECK(hipEventRecord(ev[0], d.stream));
    // S0: the undamped Schur phase (it also leaves V+ = vlg_pinv3(V) in d.Vinv),
    // dense lower triangle, unit diagonal on the exactly-zero rows
    TRY_RC(schur_phase(c, 0.0));
    TRY_RC(ba_launch_assemble_plain(&d, S, ld, 1));
    TRY_RC(ba_cov_mark_fixed(&d, S, ld, s.fixed));
    TRY_RC(ba_fix_diag_plain(&d, S, ld));
    // the library stream is non-blocking: S0 complete before rocSOLVER
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        int pinfo = 0;
        if (rs->set_stream(hdl, d.stream) != rocblas_status_success) return VLGBA_E_ARG;
        for (auto fn : {rs->potrf, rs->potri}) {
            TRY_RC(rs_factor_info(c, hdl, fn, &pinfo));
            if (pinfo != 0) return VLGBA_E_SINGULAR;
        }
    }
    TRY_RC(ba_cov_finish(&d, S, ld, s.fixed, s.diag));
    if (s.src_packed) TRY_RC(ba_cov_pack(&d, S, ld, s.bj, s.col, d.nb, s.packed));
    VLGBA_CHECK(hipEventRecord(ev[1], d.stream));
    TRY_RC(cov_points(
        c, s, ba_cov_src{S, ld, s.rowptr, s.col, s.src_packed ? s.packed.get() : nullptr}));
    VLGBA_CHECK(hipEventRecord(ev[2], d.stream));
    if (!s.src_packed)   // (for vlgba_get_covariance_blocks only)
        TRY_RC(ba_cov_pack(&d, S, ld, s.bj, s.col, d.nb, s.packed));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

// everything on the device: the setups of the first call, the linearisation,
// Sigma_a's blocks and the points' Sigma_b; ms[2]: the camera and point parts
int cov_compute(vlgba_ctx *c, ba_cov_state &s, float ms[2])
{
    ba_dev &d = c->d;
    const bool sel = s.method == VLGBA_COV_SELECTED;
    rs_api *rs = nullptr;
    rocblas_handle hdl = nullptr;
    if (!sel) {   // (the selected method needs neither rocSOLVER nor the dense scratch)
        TRY_RC(rs_prepare(d.device, &rs, &hdl));
        if (!rs->potrf || !rs->potri) return VLGBA_E_ARG;
        TRY_RC(c->dense.ensure(d.ld));
    }
    TRY_RC(cov_setup(c, s));
    if (sel) TRY_RC(cov_setup_selected(c, s));
    s.have = 0;
    TRY_RC(stage1(c, 0, CAMRED_PLAIN, nullptr));
    cov_events t;
    TRY_RC(t.create());
    const int rc = sel ? cov_run_selected(c, s, t.ev) : cov_run_dense(c, s, rs, hdl, t.ev);
    if (rc) {   // nothing queued reads the events or the buffers after this
        (void)hipStreamSynchronize(d.stream);
        return rc;
    }
    (void)hipEventElapsedTime(&ms[0], t.ev[0], t.ev[1]);
    (void)hipEventElapsedTime(&ms[1], t.ev[1], t.ev[2]);
    return 0;
}

int cov_run(vlgba_ctx *c, int scale, double *cov_a, double *cov_a_full, double *cov_b,
            double *info)
{
    ba_dev &d = c->d;
    ba_cov_state *sp = cov_state(c);
    if (!sp) return VLGBA_E_NOMEM;
    ba_cov_state &s = *sp;
    const bool sel = s.method == VLGBA_COV_SELECTED;
    const long long ld = d.ld;
    float ms[2] = {0.f, 0.f};
    TRY_RC(cov_compute(c, s, ms));
    // SSE / dof: the linearisation's SSE (the old SSE of a pass from here)
    double sse = 0.0;
    std::vector<unsigned char> fixed((size_t)ld);
    TRY_RC(download(&sse, d.eA + d.ld, 1, d.stream));
    TRY_RC(download(fixed.data(), s.fixed.get(), (size_t)ld, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    long long nfixed = 0;
    for (unsigned char f : fixed) nfixed += f;
    const double dof = 2.0 * (double)d.N -
                       ((double)(ld - nfixed) + (c->flags.fix_structure ? 0.0 : 3.0 * s.seen));
    const double sigma2 = dof > 0 ? sse / dof : 0.0;
    if (info) {
        const double scratch = sel ? 8.0 * 3.0 * 32.0 * 32.0 * (double)d.chol->plan.nt32
                                   : 8.0 * (double)ld * (double)ld;
        const double v[8] = {sse, dof, sigma2, (double)nfixed, ms[0], ms[1], scratch, 0.0};
        std::memcpy(info, v, sizeof v);
    }
    if (scale && !(dof > 0)) return VLGBA_E_ARG;
    const size_t na2m = (size_t)d.na * d.na * d.m;
    if (cov_a) TRY_RC(download(cov_a, s.diag.get(), na2m, d.stream));
    if (cov_a_full) TRY_RC(download(cov_a_full, c->dense.S.get(), (size_t)(ld * ld), d.stream));
    if (cov_b) TRY_RC(download_points(c, cov_b, s.pts, 9));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    s.have = 1;
    s.scale = scale ? sigma2 : 1.0;
    if (scale) {
        for (size_t q = 0; cov_a && q < na2m; q++) cov_a[q] *= sigma2;
        for (size_t q = 0; cov_a_full && q < (size_t)(ld * ld); q++) cov_a_full[q] *= sigma2;
        for (size_t q = 0; cov_b && q < 9 * (size_t)d.n; q++) cov_b[q] *= sigma2;
    }
    return 0;
}

// the selected method runs on the camera-aligned cyclic reduction's factors
bool cov_selected_ok(const vlgba_ctx *c)
{
    const ba_chol *ch = c->d.chol;   // (null in a stage-mode context: no factors)
    return ch && ch->plan.cr_nlev > 0 && ch->plan.cr32 && c->world == 1 && !c->comm &&
           !c->host_allreduce && !c->d.ordered;
}

}   // namespace

extern "C" {

int vlgba_covariance(vlgba_ctx *c, int scale, double *cov_a, double *cov_a_full, double *cov_b,
                     double *info)
{
    if (!c) return VLGBA_E_ARG;
    // one rank only: the sharded form (an all-reduce of S0 and per-rank point
    // blocks) is not built, and no collective runs here
    if (c->world > 1 || c->comm || c->host_allreduce) return VLGBA_E_ARG;
    // sigma2 from a robust cost is not the noise variance: unscaled only
    if (scale && c->d.loss_kind) return VLGBA_E_ARG;
    // the full matrix is the dense method's
    if (cov_a_full && c->cov && c->cov->method == VLGBA_COV_SELECTED) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    // the call's launches stay out of the pass timers
    const int timing = c->timing;
    const int kt_on = c->d.kt ? c->d.kt->on : 0;
    c->timing = 0;
    if (c->d.kt) c->d.kt->on = 0;
    const int rc = cov_run(c, scale, cov_a, cov_a_full, cov_b, info);
    c->timing = timing;
    if (c->d.kt) c->d.kt->on = kt_on;
    return rc;
}

int vlgba_set_covariance_method(vlgba_ctx *c, int kind)
{
    if (!c || (kind != VLGBA_COV_DENSE && kind != VLGBA_COV_SELECTED)) return VLGBA_E_ARG;
    if (kind == VLGBA_COV_SELECTED && !cov_selected_ok(c)) return VLGBA_E_ARG;
    if (!c->cov && kind == VLGBA_COV_DENSE) return 0;   // (the default)
    ba_cov_state *s = cov_state(c);
    if (!s) return VLGBA_E_NOMEM;
    s->method = kind;
    return 0;
}

int vlgba_get_covariance_method(vlgba_ctx *c, int *kind)
{
    if (!c || !kind) return VLGBA_E_ARG;
    *kind = c->cov ? c->cov->method : VLGBA_COV_DENSE;
    return 0;
}

int vlgba_get_covariance_blocks(vlgba_ctx *c, int *blk_jk, double *blocks)
{
    if (!c || !c->cov || !c->cov->have) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    ba_dev &d = c->d;
    const ba_cov_state &s = *c->cov;
    const size_t nn = (size_t)d.na * d.na;
    if (blk_jk) TRY_RC(download(blk_jk, d.blk_jk, 2 * (size_t)d.nb, d.stream));
    std::vector<double> pk(blocks ? nn * d.nb : 0);
    if (blocks) TRY_RC(download(pk.data(), s.packed.get(), pk.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    // packed block p (by camera row, columns ascending) is block ord[p]
    for (int p = 0; blocks && p < d.nb; p++) {
        double *o = blocks + nn * (size_t)s.ord[p];
        for (size_t q = 0; q < nn; q++) o[q] = pk[nn * p + q] * s.scale;
    }
    return 0;
}

}   // extern "C"
