// ba_solver.cpp -- libvlgba host side: problem setup, the LM driver of
// toolbox/bundle/bundle_euclid.m:111-249 and the C ABI of include/vlgba.h.
//
// The LM control flow stays on the host (it is a handful of scalars per pass,
// exactly as bundle_euclid.m keeps it in MATLAB); every array stays in HBM.
// One pass = rotations + linearize + camera reduce (skipped after a rejected
// step: bundle_euclid.m:139 recomputes an identical linearisation, App. A Q12)
// + damping/Y + Schur + dense Cholesky solve + update/new cost, then ONE
// device->host copy of 5 scalars.
//
// Multi-GPU (one process per GPU): points are split into
// contiguous ranges of balanced observation count; each rank linearises its
// points, RCCL all-reduces U/eA/old-SSE once per linearisation and the packed
// co-visible blocks of S + e_ once per pass, every rank runs the identical
// dense solve, and a 3-scalar all-reduce drives the accept/reject decision.
//
// The process-wide resources a context draws on are ba_runtime.cpp's, the
// covariance driver ba_cov_host.cpp's, the MEX stage entries ba_mex.cpp's; the
// context itself and what these units share: ba_ctx.h.
#include "ba_ctx.h"
#include "ba_plan.h"   // the host planner: sort_obs, order_points_by_kind, plan_host
#include "ba_chol.h"   // the reduced solve's state and plan (ba_dev::chol)
#include "ba_pcg.h"    // ... or the block-Jacobi PCG's (ba_dev::pcg)

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#define VLGBA_STR2(x) #x
#define VLGBA_STR(x) VLGBA_STR2(x)
#define VLGBA_VERSION_STR \
    "vlgba 0.2 (abi " VLGBA_STR(VLGBA_ABI_VERSION) ", gfx950, fp64, MFMA-f64 Cholesky)"

// Order: both streams drain, then the device memory of ctx_alloc goes, the
// timers retire, the reduced solve's state, the communicator and the pooled
// streams are given back; the members that own device memory themselves (the
// dense scratch, the covariance state: ba_dbuf) go last, with the context.
// Nothing is queued on the streams by then.
void ctx_free(vlgba_ctx *c)
{
    if (!c) return;
    if (c->d.stream) (void)hipStreamSynchronize(c->d.stream);
    if (c->d.side) (void)hipStreamSynchronize(c->d.side);
    for (void *p : c->allocs) ba_dfree(p);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->d.kt) {
        kt_retire(c->d.kt);
        for (int q = 0; q < c->d.kt->ncreated; q++) (void)hipEventDestroy(c->d.kt->ev[q]);
        delete c->d.kt;
    }
    ba_chol_free(&c->d);
    ba_pcg_free(&c->d);
    if (c->comm) comm_release(c->comm);
    if (c->has_aux) aux_release(c->aux);
    delete c;
}

int ba_dense::ensure(long long ld)
{
    if (info) return 0;   // (allocated last)
    if (ld > 0x7fffffffLL) return VLGBA_E_ARG;
    TRY_RC(S.alloc((size_t)(ld * ld)));
    TRY_RC(ev.alloc((size_t)ld));
    TRY_RC(e.alloc((size_t)ld));
    TRY_RC(w.alloc((size_t)ld));
    return info.alloc(1);
}

// a device temporary of one call: the stream it was used on drains before the
// block goes, on every path
template <typename T>
struct ba_dtmp : ba_dbuf<T> {
    hipStream_t s;
    explicit ba_dtmp(hipStream_t s_) : s(s_) {}
    ~ba_dtmp()
    {
        if (this->get()) (void)hipStreamSynchronize(s);
    }
};

static int allreduce(vlgba_ctx *c, double *buf, size_t count)
{
    if ((c->world <= 1 && !c->comm) || count == 0) return 0;
    if (c->comm) {
        ncclResult_t r =
            ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, c->comm, c->d.stream);
        return r == ncclSuccess ? 0 : VLGBA_E_COMM;
    }
    // host collective (vlgba_options.allreduce): device -> host, sum, host -> device
    c->hb_tmp.resize(count);
    TRY_RC(download(c->hb_tmp.data(), buf, count, c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    if (c->host_allreduce(c->hb_tmp.data(), (long long)count, c->host_user) != 0)
        return VLGBA_E_COMM;
    TRY_RC(upload(buf, c->hb_tmp.data(), count, c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

// setup timing trace (VLGBA_SETUP_TRACE=1: one stderr line per context)
struct setup_trace {
    bool on = std::getenv("VLGBA_SETUP_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    std::string line;
    void mark(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[64];
        std::snprintf(buf, sizeof buf, " %s=%.0fus", what,
                      std::chrono::duration<double, std::micro>(now - t).count());
        line += buf;
        t = now;
    }
    ~setup_trace()
    {
        if (on && !line.empty()) std::fprintf(stderr, "[vlgba setup]%s\n", line.c_str());
    }
};
static thread_local setup_trace *g_st = nullptr;
#define ST_MARK(w) do { if (g_st) g_st->mark(w); } while (0)

// A context's plan arrays (~30 host vectors) go to the device as ONE copy:
// each array at a 256-byte aligned offset of one device block and of the
// context's pinned staging buffer (ba_aux::pin, which set_params reuses) --
// one hipMemcpyAsync from pinned memory instead of one pageable copy per
// array (the setup trace's plan_upload: 1.1 ms per context over the growing
// replay, profiles/r06/r06f_cfg5x_setup_phases.txt).  The pointers stay valid
// for the context's life (the block is one of its allocations).
struct plan_batch {
    struct item {
        void **dst;
        const void *src;
        size_t bytes, off;
    };
    std::vector<item> items;
    size_t total = 0;
    template <typename T> void add(T **dst, const std::vector<T> &v)
    {
        items.push_back({(void **)dst, v.data(), sizeof(T) * v.size(), total});
        total += (sizeof(T) * std::max<size_t>(v.size(), 1) + 255) & ~(size_t)255;
    }
    int commit(vlgba_ctx *c, hipStream_t s)
    {
        if (items.empty()) return 0;
        char *dev = nullptr;
        TRY_RC(ctx_alloc(c, &dev, total));
        char *stage = (char *)aux_pin(c->aux, (total + sizeof(double) - 1) / sizeof(double));
        for (const item &it : items) {
            *it.dst = dev + it.off;
            if (it.bytes == 0) continue;
            if (stage)
                std::memcpy(stage + it.off, it.src, it.bytes);
            else   // (no pinned memory: array by array)
                VLGBA_CHECK(hipMemcpyAsync(dev + it.off, it.src, it.bytes,
                                           hipMemcpyHostToDevice, s));
        }
        if (stage)
            VLGBA_CHECK(hipMemcpyAsync(dev, stage, total, hipMemcpyHostToDevice, s));
        VLGBA_CHECK(hipStreamSynchronize(s));
        return 0;
    }
};

// ---------------------------------------------------------------------------
// context setup: ctx_setup plans, allocates and uploads for the observations of
// points [p0, p1); the pieces below run in its order and nowhere else
// ---------------------------------------------------------------------------
// this rank's point-major arrays and the camera-major view of its observations
// (obs ids ascending per camera)
struct local_lists {
    std::vector<int> lptr, lcam, cptr, cobs;
};

static void setup_local_lists(const ba_dev &d, const host_obs &h,
                              const std::vector<int> &pt_ptr_all, int p0, long long o0,
                              long long o1, local_lists &L)
{
    L.lptr.resize(d.n + 1);
    L.lcam.assign(h.cam.begin() + o0, h.cam.begin() + o1);
    for (int i = 0; i <= d.n; i++) L.lptr[i] = pt_ptr_all[p0 + i] - (int)o0;
    L.cptr.assign(d.m + 1, 0);
    L.cobs.resize(d.N);
    for (int o = 0; o < d.N; o++) L.cptr[L.lcam[o] + 1]++;
    for (int j = 0; j < d.m; j++) L.cptr[j + 1] += L.cptr[j];
    std::vector<int> pos(L.cptr.begin(), L.cptr.end() - 1);
    for (int o = 0; o < d.N; o++) L.cobs[pos[L.lcam[o]]++] = o;
}

// the fast path's plan on the device: its scalars, the buffers sized by it, and
// its arrays as one block and one copy (plan_batch)
static int setup_fast_plan(vlgba_ctx *c, const host_plan &plan, const local_lists &L, int p_long)
{
    ba_dev &d = c->d;
    const int na = d.na;
    d.nch_reg = plan.nch_reg;
    d.nch = plan.nch_reg + plan.nseg;
    d.nl = (int)plan.long_pt.size();
    d.max_lcam = plan.max_lcam;
    d.long_o0_h = plan.long_o0.empty() ? 0 : plan.long_o0[0];
    d.p_long = p_long;
    plan_batch pb;
    if (d.nl > 0) {
        pb.add(&d.seg_pt, plan.seg_pt);
        pb.add(&d.seg_long, plan.seg_long);
        pb.add(&d.long_pt, plan.long_pt);
        pb.add(&d.long_o0, plan.long_o0);
        pb.add(&d.long_seg0, plan.long_seg0);
        pb.add(&d.long_ebase, plan.long_ebase);
        pb.add(&d.cam_lptr, plan.cam_lptr);
        pb.add(&d.cam_lobs, plan.cam_lobs);
        pb.add(&d.cam_ltrk, plan.cam_ltrk);
        TRY_RC(ctx_alloc(c, &d.ylong, (size_t)3 * na * plan.cam_lobs.size()));
        TRY_RC(ctx_alloc(c, &d.vseg, 12 * (size_t)plan.nseg));
        TRY_RC(ctx_alloc(c, &d.dpg_long, (size_t)d.nl));
    }
    d.ns = (int)plan.slot_blk.size();
    d.nes = (int)plan.eslot_optr.size() - 1;
    d.ch_max_terms = plan.max_terms;
    d.ch_max_slots = plan.max_slots;
    d.nterm_fast = plan.n_terms;
    d.blob_words = (long long)plan.blob.size();
    d.ngrp = (int)plan.grp_ch.size() - 1;
    d.ngrp_mf = plan.ngrp_mf;
    d.max_blob = plan.max_blob;
    d.mf_max_blob = plan.mf_max_blob;
    d.mf_max_s = plan.mf_max_s;
    d.mf_max_e = plan.mf_max_e;
    // V*^-1 inside k_schur_mfma when the MFMA groups tile every point
    const char *vf = std::getenv("VLGBA_VINV_FOLD");   // read per context (tests)
    d.vinv_fold = plan_mfma_groups_tile_points(plan, d.n) && !(vf && vf[0] == '0');
    pb.add(&d.blob, plan.blob);
    pb.add(&d.ch_blob, plan.ch_blob);
    pb.add(&d.ch_obase, plan.ch_obase);
    // chunk-local point of every observation (k_linearize_chunk) and each
    // chunk's camera range (k_update_linearize's da staging)
    std::vector<unsigned char> lpt;
    std::vector<int> ccam;
    plan_obs_local_point(plan, L.lptr, lpt);
    plan_chunk_cameras(plan, L.lcam, ccam);
    // VLGBA_DA_STAGE=0 (A/B): every range too wide, each lane loads its da row
    const char *dse = std::getenv("VLGBA_DA_STAGE");
    if (dse && dse[0] == '0')
        for (size_t ch = 0; ch + 1 < plan.ch_obase.size(); ch++)
            ccam[2 * ch + 1] = ccam[2 * ch] + (1 << 20);
    pb.add(&d.obs_lpt, lpt);
    pb.add(&d.ch_cam, ccam);
    d.grp_max_s = plan.grp_max_s;
    d.grp_max_e = plan.grp_max_e;
    d.ngs = (int)plan.gslot_blk.size();
    d.nge = (int)plan.gecam.size();
    TRY_RC(ctx_alloc(c, &d.spart, (size_t)na * na * d.ngs));
    TRY_RC(ctx_alloc(c, &d.epart, (size_t)na * d.nge));
    pb.add(&d.grp_ch, plan.grp_ch);
    pb.add(&d.grp_gs, plan.grp_gs);
    pb.add(&d.grp_ge, plan.grp_ge);
    pb.add(&d.cs_g, plan.cs_g);
    pb.add(&d.ce_g, plan.ce_g);
    pb.add(&d.blk_gptr, plan.blk_gptr);
    pb.add(&d.blk_gslots, plan.blk_gslots);
    pb.add(&d.cam_gptr, plan.cam_gptr);
    pb.add(&d.cam_gslots, plan.cam_gslots);
    TRY_RC(ctx_alloc(c, &d.upart, (size_t)(na * (na + 1) / 2 + na) * d.nes));
    TRY_RC(ctx_alloc(c, &d.chsse, 3 * (size_t)d.nch));   // lin SSE | new SSE | dpg
    pb.add(&d.ch_pt, plan.ch_pt);
    pb.add(&d.ch_eslot, plan.ch_eslot);
    pb.add(&d.eslot_optr, plan.eslot_optr);
    pb.add(&d.eslot_obs, plan.eslot_obs);
    pb.add(&d.cam_eptr, plan.cam_eptr);
    pb.add(&d.cam_eslots, plan.cam_eslots);
    TRY_RC(pb.commit(c, d.stream));   // (synchronous: the plan vectors are thread scratch)
    ST_MARK("plan_upload");
    return 0;
}

// the problem's arrays and this rank's state and linearisation.  W, eB, V*^-1
// carry one zero row past the end: the MFMA Schur kernel points the fragment
// loads of absent (point, camera) pairs at it
static int setup_state_allocs(vlgba_ctx *c)
{
    ba_dev &d = c->d;
    const size_t m = (size_t)d.m;
    TRY_RC(ctx_alloc(c, &d.obs_cam, d.N));
    TRY_RC(ctx_alloc(c, &d.pt_ptr, d.n + 1));
    TRY_RC(ctx_alloc(c, &d.cam_ptr, d.m + 1));
    TRY_RC(ctx_alloc(c, &d.cam_obs, d.N));
    TRY_RC(ctx_alloc(c, &d.obs_x, 2 * (size_t)d.N));
    TRY_RC(ctx_alloc(c, &d.K4, 4 * m));
    TRY_RC(ctx_alloc(c, &d.a, (size_t)d.ld));
    TRY_RC(ctx_alloc(c, &d.a_new, (size_t)d.ld));
    TRY_RC(ctx_alloc(c, &d.b, 3 * (size_t)d.n));
    TRY_RC(ctx_alloc(c, &d.b_new, 3 * (size_t)d.n));
    TRY_RC(ctx_alloc(c, &d.rot, 45 * m));
    TRY_RC(ctx_alloc(c, &d.rot_new, 45 * m));
    TRY_RC(ctx_alloc(c, &d.W, (size_t)3 * d.na * (d.N + 1)));
    VLGBA_CHECK(hipMemsetAsync(d.W + (size_t)3 * d.na * d.N, 0, sizeof(double) * 3 * d.na,
                               d.stream));
    return 0;
}

// U / eA, the points' blocks, and the fused update's second buffers
static int setup_lin_allocs(vlgba_ctx *c, bool fast)
{
    ba_dev &d = c->d;
    const int na = d.na;
    hipStream_t s = d.stream;
    TRY_RC(ctx_alloc(c, &d.U, (size_t)na * na * d.m + na * (size_t)d.m + 1));
    d.eA = d.U + (size_t)na * na * d.m;     // U | eA | old_sse contiguous: one all-reduce
    TRY_RC(ctx_alloc(c, &d.V, 9 * (size_t)d.n));
    TRY_RC(ctx_alloc(c, &d.eB, 3 * (size_t)(d.n + 1)));
    TRY_RC(ctx_alloc(c, &d.Vinv, 9 * (size_t)(d.n + 1)));
    VLGBA_CHECK(hipMemsetAsync(d.eB + 3 * (size_t)d.n, 0, sizeof(double) * 3, s));
    VLGBA_CHECK(hipMemsetAsync(d.Vinv + 9 * (size_t)d.n, 0, sizeof(double) * 9, s));
    TRY_RC(ctx_alloc(c, &d.db, 3 * (size_t)d.n));
    // fused update (fast path): the next linearisation's buffers (VLGBA_FUSED=0
    // keeps the separate update and linearisation launches: A/B)
    const char *fused_env = std::getenv("VLGBA_FUSED");   // read per context (tests)
    const bool fused_on = !(fused_env && fused_env[0] == '0');
    if (fast && d.nch > 0 && fused_on) {
        TRY_RC(ctx_alloc(c, &d.W2, (size_t)3 * na * (d.N + 1)));
        VLGBA_CHECK(hipMemsetAsync(d.W2 + (size_t)3 * na * d.N, 0, sizeof(double) * 3 * na, s));
        TRY_RC(ctx_alloc(c, &d.V2, 9 * (size_t)d.n));
        TRY_RC(ctx_alloc(c, &d.eB2, 3 * (size_t)(d.n + 1)));
        VLGBA_CHECK(hipMemsetAsync(d.eB2 + 3 * (size_t)d.n, 0, sizeof(double) * 3, s));
        TRY_RC(ctx_alloc(c, &d.upart2, (size_t)(na * (na + 1) / 2 + na) * d.nes));
        TRY_RC(ctx_alloc(c, &d.chsse2, 3 * (size_t)d.nch));
        d.fused = 1;
    }
    return 0;
}

// The long tracks' per-block pair lists (k_long_pairs), in two halves.
// fill = 0: the pair counts per block into *cnt, on the device while the host
// builds the solve's structure (chol_plan_build).  fill = 1, after the uploads:
// the counts read back and summed, the pairs written, and the blocks with
// pairs listed for k_schur_long_acc, most pairs first
static int setup_long_pairs(vlgba_ctx *c, int fill, int **cnt)
{
    ba_dev &d = c->d;
    hipStream_t s = d.stream;
    if (!fill) {
        TRY_RC(ctx_alloc(c, cnt, (size_t)d.nb + 1));
        TRY_RC(ctx_alloc(c, &d.lpair_ptr, (size_t)d.nb + 1));
        return ba_launch_long_pairs(&d, 0, *cnt);
    }
    std::vector<int> h((size_t)d.nb + 1, 0);
    TRY_RC(download(h.data(), *cnt, (size_t)d.nb, s));
    VLGBA_CHECK(hipStreamSynchronize(s));
    long long tot = 0;
    for (int b = 0; b < d.nb; b++) {
        const int v = h[b];
        h[b] = (int)tot;
        tot += v;
    }
    h[d.nb] = (int)tot;
    if (tot > 0x7fffffffLL) return VLGBA_E_ARG;
    TRY_RC(ctx_alloc(c, &d.lpair, (size_t)tot + 1));
    TRY_RC(upload(d.lpair_ptr, h.data(), (size_t)d.nb + 1, s));
    TRY_RC(ba_launch_long_pairs(&d, 1, nullptr));
    // (VLGBA_LONG_ACC=0: k_schur_reduce streams the pairs itself)
    const char *la = std::getenv("VLGBA_LONG_ACC");
    if (!(la && la[0] == '0')) {
        std::vector<int> lb;
        for (int b = 0; b < d.nb; b++)
            if (h[b + 1] > h[b]) lb.push_back(b);
        std::stable_sort(lb.begin(), lb.end(),
                         [&](int x, int y) { return h[x + 1] - h[x] > h[y + 1] - h[y]; });
        d.nlb = (int)lb.size();
        if (d.nlb > 0) {
            TRY_RC(ctx_alloc(c, &d.lblk, lb.size()));
            TRY_RC(upload(d.lblk, lb.data(), lb.size(), s));
        }
    }
    ST_MARK("long_pairs");
    return 0;
}

// the two decisions a pass takes from the reduced solve's plan
struct solve_decisions {
    int asm_direct, camupd_fold;
};
static solve_decisions setup_solve_decisions(const vlgba_ctx *c, bool fast)
{
    const ba_dev &d = c->d;
    const chol_plan &P = d.chol->plan;
    const bool cr32 = fast && !d.ordered && P.cr_nlev > 0 && P.cr32 && P.nd_np == 0;
    // direct assembly (ba_dev::asm_direct): one rank without a collective
    // between the block sums and the solve, the fast path's block sums, no
    // long tracks (k_schur_long_acc adds to the sums after them);
    // VLGBA_ASM_DIRECT=0 keeps k_assemble_tiles (A/B)
    const char *ad = std::getenv("VLGBA_ASM_DIRECT");
    const int asm_direct = P.asm_direct_ok && !(ad && ad[0] == '0') && cr32 && c->world == 1 &&
                           !c->comm && d.nl == 0;
    // camera update inside the one-launch CR (ba_dev::camupd_fold): x = da
    // in camera order, every tile a whole number of cameras, the Euclidean
    // models' rotation table, the fast path's final sums (k_sum_parts3);
    // VLGBA_CAMUPD_FOLD=0 keeps k_camera_update (A/B, tests)
    const char *cf = std::getenv("VLGBA_CAMUPD_FOLD");
    const int camupd_fold = !(cf && cf[0] == '0') && cr32 && d.nch > 0 && P.cr_fused &&
                            d.chol->crflag && d.na != BA_PROJ_NA && d.na <= 10 &&
                            P.tb32 % d.na == 0 && d.ld == (long long)d.na * d.m;
    return {asm_direct, camupd_fold};
}

// blocks | rhs | old SSE contiguous (one all-reduce per pass, world > 1), da,
// and the reduced solve the context runs: the PCG on sblk / rhs themselves (no
// dense S, no plan of the direct solves: d.chol stays null, no direct assembly,
// no folded camera update), the direct solves' plan, or none (stage mode)
static int setup_solve(vlgba_ctx *c, const host_blocks &hb, bool stage_mode, bool fast)
{
    ba_dev &d = c->d;
    TRY_RC(ctx_alloc(c, &d.sblk, (size_t)d.na * d.na * d.nb + d.lds + 1));
    d.rhs = d.sblk + (size_t)d.na * d.na * d.nb;
    TRY_RC(ctx_alloc(c, &d.da, (size_t)d.lds));   // S, linv, ywork: ba_chol_setup
    if (stage_mode) return 0;
    ST_MARK("allocs");
    if (d.dense_solve == 5) {
        TRY_RC(ba_pcg_setup(&d, hb.jk.data(), d.nb));
        ST_MARK("pcg_setup");
        return 0;
    }
    TRY_RC(ba_chol_setup(&d, hb.jk.data(), d.nb));
    ST_MARK("chol_setup");
    const solve_decisions dec = setup_solve_decisions(c, fast);
    d.asm_direct = dec.asm_direct;
    d.camupd_fold = dec.camupd_fold;
    return 0;
}

static int setup_uploads(vlgba_ctx *c, const vlgba_problem *p, const host_obs &h,
                         const local_lists &L, const host_blocks &hb, long long o0)
{
    ba_dev &d = c->d;
    hipStream_t s = d.stream;
    TRY_RC(upload(d.obs_cam, L.lcam.data(), d.N, s));
    TRY_RC(upload(d.pt_ptr, L.lptr.data(), d.n + 1, s));
    TRY_RC(upload(d.cam_ptr, L.cptr.data(), p->m + 1, s));
    TRY_RC(upload(d.cam_obs, L.cobs.data(), d.N, s));
    TRY_RC(upload(d.obs_x, h.x.data() + 2 * o0, 2 * (size_t)d.N, s));
    if (p->K) TRY_RC(upload(d.K4, p->K, 4 * (size_t)p->m, s));
    else VLGBA_CHECK(hipMemsetAsync(d.K4, 0, sizeof(double) * 4 * p->m, s));
    TRY_RC(upload(d.blk_ptr, hb.ptr.data(), hb.ptr.size(), s));
    TRY_RC(upload(d.term, hb.term.data(), hb.term.size(), s));
    ST_MARK("uploads");
    return 0;
}

// Device buffers + host-side structure for the observations of points [p0, p1).
static int ctx_setup(vlgba_ctx *c, const vlgba_problem *p, const host_obs &h,
                     const std::vector<int> &pt_ptr_all, bool lower_blocks, bool all_diag,
                     bool stage_mode)
{
    ba_dev &d = c->d;
    const int na = p->num_a;
    d.device = c->aux.device;
    VLGBA_CHECK(hipDeviceGetAttribute(&d.ncu, hipDeviceAttributeMultiprocessorCount, d.device));
    d.m = p->m;
    d.na = na;
    d.js = 2 * na + 2;
    d.n = c->p1 - c->p0;
    const long long o0 = pt_ptr_all[c->p0], o1 = pt_ptr_all[c->p1];
    d.N = (int)(o1 - o0);
    d.ld = (long long)na * p->m;
    d.lds = ((d.ld + 63) / 64) * 64;
    // every rank adds its own partial U* / eA into its partial reduced system
    // (the damping is linear: sum_r (1 + lambda) U_r = (1 + lambda) sum_r U_r),
    // so U / eA never need an all-reduce of their own; the camera part of
    // dp'(lambda dp + g) takes its lambda dp'dp term from rank 0 only
    d.schur_owner = 1;
    d.dpg_lambda = c->rank == 0;
    hipStream_t s = d.stream;

    local_lists L;
    setup_local_lists(d, h, pt_ptr_all, c->p0, o0, o1, L);
    bool fast = !d.ordered && !stage_mode;
    int p_long = d.n;
    // the host plan in this thread's scratch: its storage is kept from one
    // context to the next (the growing replay creates one per solve on its two
    // prefetch workers)
    static thread_local host_blocks hb;
    static thread_local host_plan plan;
    hb.reset();
    plan.reset();
    ST_MARK("lists");
    plan_host(p->m, na, d.n, L.lptr, L.lcam, pt_ptr_all, h.cam, c->p0, c->p1, o0, lower_blocks,
              all_diag, d.no_mfma != 0, fast, p_long, hb, plan,
              [](const char *w) { ST_MARK(w); });
    d.mfma = fast && plan.nch_mf > 0;
    if (!fast) d.ordered = 1;
    // the ordered kernels read the table's slots 1..4 as R(w + h e_k): a context
    // the planner hands to them keeps the forward differences, whatever
    // VLGBA_JACOBIAN asked for (vlgba_set_jacobian refuses it afterwards)
    if (d.ordered) d.jac = VLGBA_JAC_FD;
    ST_MARK("plan");
    d.nb = (int)hb.jk.size() / 2;
    d.T = (long long)hb.term.size() / 2;

    TRY_RC(setup_state_allocs(c));
    if (!fast) {   // the fast path forms A, e, Y and t in LDS only
        TRY_RC(ctx_alloc(c, &d.jrec, (size_t)d.js * d.N));
        TRY_RC(ctx_alloc(c, &d.Y, (size_t)3 * na * d.N));
        TRY_RC(ctx_alloc(c, &d.t, (size_t)na * d.N));
    } else {
        TRY_RC(setup_fast_plan(c, plan, L, p_long));
    }
    TRY_RC(setup_lin_allocs(c, fast));
    TRY_RC(ctx_alloc(c, &d.blk_jk, 2 * (size_t)d.nb));
    TRY_RC(ctx_alloc(c, &d.blk_ptr, (size_t)d.nb + 1));
    TRY_RC(ctx_alloc(c, &d.term, 2 * (size_t)d.T));
    TRY_RC(upload(d.blk_jk, hb.jk.data(), hb.jk.size(), s));
    int *lp_cnt = nullptr;
    if (fast && d.nl > 0) TRY_RC(setup_long_pairs(c, 0, &lp_cnt));
    TRY_RC(setup_solve(c, hb, stage_mode, fast));
    TRY_RC(ctx_alloc(c, &d.part, 3 * (size_t)BA_PART_MAX));
    TRY_RC(ctx_alloc(c, &d.scal, 8));
    TRY_RC(setup_uploads(c, p, h, L, hb, o0));
    if (fast && d.nl > 0) TRY_RC(setup_long_pairs(c, 1, &lp_cnt));
    VLGBA_CHECK(hipMemsetAsync(d.scal, 0, 8 * sizeof(double), s));
    TRY_RC(ctx_alloc(c, &d.pub_cnt, 1));
    VLGBA_CHECK(hipMemsetAsync(d.pub_cnt, 0, sizeof(unsigned), s));
    VLGBA_CHECK(hipStreamSynchronize(s));   // host vectors go out of scope
    return 0;
}

// ---------------------------------------------------------------------------
// context creation
// ---------------------------------------------------------------------------
static int ctx_check_problem(const vlgba_problem *p, const vlgba_options *o, bool stage_mode)
{
    if (!p || p->m < 1 || p->n < 0 || p->num_obs < 0) return VLGBA_E_ARG;
    if (p->model == VLGBA_MODEL_EUCLIDEAN) {
        if (!p->K) return VLGBA_E_ARG;
        if (p->num_a != 6 && p->num_a != 7 && p->num_a != 10 && p->num_a != BA_RAD_NA)
            return VLGBA_E_NUMA;
        // the radial model lives on the fast path alone: the stage entries do not
        // cover it, ordered / parity mode (the reference's differences) cannot
        if (p->num_a == BA_RAD_NA && stage_mode) return VLGBA_E_NUMA;
        if (p->num_a == BA_RAD_NA && o && o->ordered != 0) return VLGBA_E_ARG;
    } else if (p->model == VLGBA_MODEL_PROJECTIVE) {
        if (p->num_a != BA_PROJ_NA) return VLGBA_E_NUMA;
    } else {
        return VLGBA_E_ARG;
    }
    if (p->num_obs > 0x7fffffffLL) return VLGBA_E_ARG;
    return 0;
}

// the pooled streams / events / result block, into the context and its ba_dev
static int ctx_take_aux(vlgba_ctx *c, int device)
{
    if (hipSetDevice(device) != hipSuccess) return VLGBA_E_ARG;
    if (aux_acquire(device, c->aux)) return -1;
    c->has_aux = true;
    c->d.stream = c->aux.stream;
    c->d.side = c->aux.side;
    c->d.ev_fork = c->aux.ev_fork;
    c->d.ev_join = c->aux.ev_join;
    c->d.hres = c->aux.hres_host;
    c->d.hres_dev = c->aux.hres_dev;
    ST_MARK("aux");
    return 0;
}

// this rank's contiguous point range (balanced observation counts) and its
// collective: an RCCL communicator or the caller's host all-reduce
static int ctx_ranks(vlgba_ctx *c, const vlgba_problem *p, const vlgba_options *o,
                     const std::vector<int> &pt_ptr_all)
{
    c->world = o->world_size > 1 ? o->world_size : 1;
    c->rank = c->world > 1 ? o->rank : 0;
    if (c->world > 1) {
        const long long N = p->num_obs;
        auto bound = [&](int r) -> int {
            const long long target = (N * r) / c->world;
            return (int)(std::lower_bound(pt_ptr_all.begin(), pt_ptr_all.end(), (int)target) -
                         pt_ptr_all.begin());
        };
        c->p0 = c->rank == 0 ? 0 : std::min(bound(c->rank), p->n);
        c->p1 = c->rank == c->world - 1 ? p->n : std::min(bound(c->rank + 1), p->n);
        if (o->comm_id) {
            if (comm_acquire(&c->comm, c->world, o->comm_id, c->rank) != ncclSuccess)
                return VLGBA_E_COMM;
        } else if (o->allreduce) {
            c->host_allreduce = o->allreduce;
            c->host_user = o->allreduce_user;
        } else {
            return VLGBA_E_COMM;
        }
        return 0;
    }
    c->p0 = 0;
    c->p1 = p->n;
    // a one-rank RCCL communicator: every collective of the pass runs through
    // RCCL (identity sums)
    if (o->comm_id && comm_acquire(&c->comm, 1, o->comm_id, 0) != ncclSuccess)
        return VLGBA_E_COMM;
    return 0;
}

// the options into the context (before ctx_setup, which reads them)
static int ctx_options(vlgba_ctx *c, const vlgba_problem *p, const vlgba_options *o,
                       bool stage_mode)
{
    c->n_global = p->n;
    c->N_global = p->num_obs;
    c->num_vis = p->num_vis > 0 ? p->num_vis : (double)p->num_obs;
    c->flags.fix_structure = o->fix_structure;
    c->flags.fix_motion = o->fix_motion;
    if (o->semantics != 0 && o->semantics != 1) return VLGBA_E_ARG;
    // bundle_euclid_nomex.m has no fix_pivot option: the pivot is ignored there
    // (nor has bundle_projective.m, :46-56)
    c->flags.has_pivot = o->pivot != nullptr && o->semantics == 0 &&
                         p->model == VLGBA_MODEL_EUCLIDEAN;
    c->model = p->model;
    c->max_iter = o->max_iter > 0 ? o->max_iter : 20;
    c->max_iter2 = o->max_iter2 > 0 ? o->max_iter2 : 10;
    c->lambda0 = c->lambda = o->lambda0 > 0 ? o->lambda0 : 1e-3;
    c->verbose = o->verbose;
    c->d.dense_solve = o->dense_solve;
    c->d.ordered = o->ordered != 0;
    // the PCG (dense_solve = 5) is the fast path's: not with ordered / parity
    if (o->dense_solve == 5 && (o->ordered != 0 || stage_mode)) return VLGBA_E_ARG;
    if (o->ordered == 2) {   // parity mode: + sequential solve and LM scalars
        if (c->world > 1) return VLGBA_E_ARG;
        c->d.parity = 1;
        c->d.dense_solve = 3;
    } else if (o->ordered < 0 || o->ordered > 2 || o->dense_solve < 0 || o->dense_solve > 5) {
        return VLGBA_E_ARG;
    }
    c->stop_rel = o->stop_rel > 0 ? o->stop_rel : 1e-3;
    if (const char *ev = std::getenv("VLGBA_DEBUG_SPIN_TIMEOUT")) {
        // "R:K": rank R's first K passes report a hand-off timeout (tests)
        int r = -1, k = 0;
        if (std::sscanf(ev, "%d:%d", &r, &k) == 2 && r == c->rank) c->debug_timeouts = k;
        // a leftover variable would silently force re-solves: say so
        if (c->debug_timeouts > 0)
            std::fprintf(stderr, "[vlgba] VLGBA_DEBUG_SPIN_TIMEOUT=%s: rank %d's first %d "
                         "passes report a hand-off timeout (test hook)\n", ev, r, k);
    }
    c->on_pass = o->on_pass;
    c->on_pass_user = o->on_pass_user;
    c->d.no_mfma = o->schur_kernel == 1;
    // (the radial model has no MEX quirk to mimic: all nine rows of da)
    c->d.ndb = o->semantics == 1 || p->num_a == BA_RAD_NA ? p->num_a : 6;
    c->d.loss_kind = VLGBA_LOSS_NONE;   // vlgba_set_loss
    c->d.loss_scale = 0.0;
    c->d.jac = VLGBA_JAC_FD;            // vlgba_set_jacobian
    if (const char *ev = std::getenv("VLGBA_JACOBIAN")) {
        // the default of a fast-path context (ordered / parity and the stage
        // entries keep the reference's forward differences)
        if (!std::strcmp(ev, "analytic") && o->ordered == 0 && !stage_mode)
            c->d.jac = VLGBA_JAC_ANALYTIC;
    }
    // the radial model's Jacobian is closed form only (a difference with
    // h = 1e-10 on k1 is noise), whatever VLGBA_JACOBIAN says
    if (p->num_a == BA_RAD_NA) c->d.jac = VLGBA_JAC_ANALYTIC;
    return 0;
}

// what a context gets after ctx_setup: the refusals that need the plan, the
// parity projections, the pivot mask, the timers of VLGBA_KTIME_ALL
static int ctx_finish(vlgba_ctx *c, const vlgba_problem *p, const vlgba_options *o)
{
    // a problem the planner hands to the ordered kernels: not the radial model
    // (its Jacobian is closed form only), nor the PCG
    if (p->num_a == BA_RAD_NA && c->d.ordered) return VLGBA_E_ARG;
    if (c->d.pcg && c->d.ordered) return VLGBA_E_ARG;
    ST_MARK("setup_end");
    if (c->d.parity)   // new projections for the sequential new-SSE sum
        TRY_RC(ctx_alloc(c, &c->d.xh_out, 2 * (size_t)c->d.N + 2));
    if (c->flags.has_pivot) {
        TRY_RC(ctx_alloc(c, &c->d.pivot, (size_t)p->m));
        TRY_RC(upload(c->d.pivot, o->pivot, (size_t)p->m, c->d.stream));
    }
    if (std::getenv("VLGBA_KTIME_ALL")) TRY_RC(vlgba_set_timing(c, 1));
    return 0;
}

int ctx_create(const vlgba_problem *p, const vlgba_options *o, vlgba_ctx **out, bool lower_blocks,
               bool all_diag, bool stage_mode)
{
    *out = nullptr;
    TRY_RC(ctx_check_problem(p, o, stage_mode));
    // (before the context: its owner drains the streams while these still stand)
    host_obs h;
    std::vector<int> pt_ptr_all(p->n + 1, 0);
    ctx_ptr c(new (std::nothrow) vlgba_ctx());   // freed on every early return
    if (!c) return VLGBA_E_NOMEM;
    std::memset(&c->d, 0, sizeof(c->d));
    vlgba_options defaults;
    std::memset(&defaults, 0, sizeof defaults);
    if (!o) o = &defaults;
    setup_trace trace;
    g_st = &trace;
    struct st_reset { ~st_reset() { g_st = nullptr; } } st_reset_;
    TRY_RC(ctx_take_aux(c.get(), o->device));
    TRY_RC(sort_obs(p, h));
    ST_MARK("sort");
    for (size_t q = 0; q < h.pt.size(); q++) pt_ptr_all[h.pt[q] + 1]++;
    for (int i = 0; i < p->n; i++) pt_ptr_all[i + 1] += pt_ptr_all[i];
    TRY_RC(ctx_ranks(c.get(), p, o, pt_ptr_all));
    // fast path: this rank's points by track kind (short tracks for the MFMA
    // Schur chunks first, per-term tracks, long tracks last); the ranges
    // of the other ranks are left as they are (the block set, the only
    // global structure a rank builds, is order independent: build_blocks)
    if (o->ordered == 0 && !stage_mode)
        order_points_by_kind(o->schur_kernel == 1 ? 0 : BA_MF_CMAX(p->num_a), h, pt_ptr_all,
                             c->p0, c->p1, c->pperm, c->operm);
    ST_MARK("order");
    TRY_RC(ctx_options(c.get(), p, o, stage_mode));
    TRY_RC(ctx_setup(c.get(), p, h, pt_ptr_all, lower_blocks, all_diag, stage_mode));
    TRY_RC(ctx_finish(c.get(), p, o));
    *out = c.release();
    return 0;
}

// ---------------------------------------------------------------------------
// one LM pass
// ---------------------------------------------------------------------------
static inline void mark(vlgba_ctx *c, int q)
{
    if (c->timing) (void)hipEventRecord(c->ev[q], c->d.stream);
}

// Stage 1 at the current parameters: brings the context to "linearised, U /
// eA and the old SSE in place" (lin_valid, no camera reduction due).
// Linearises if the context holds no linearisation, or if relinearize and
// the update is not the fused one: the fused update linearises every pass at
// the new point (into the second buffers, swapped in on accept), so a pass
// linearises here only after set_params, and relinearize then means the
// camera reduction of the current linearisation (the rest of stage 1), the
// work an accepted pass does.  The rotation table of d.a is current whenever
// this runs: set_params and set_jacobian build it, an accepted step swaps in
// the one built for a_new, and nothing else writes d.a.  Only a pass routes
// the reduction off the library stream, and then passes `left` on to its
// Schur phase.
int stage1(vlgba_ctx *c, int relinearize, camred_route route, stage1_left *left)
{
    ba_dev &d = c->d;
    const bool full = !c->lin_valid || (relinearize && !d.fused);
    if (full) TRY_RC(ba_launch_linearize(&d, c->flags));
    mark(c, 1);
    if (!full && !relinearize && !c->camred_due) return 0;
    if (route == CAMRED_FOLD) {
        left->fold = true;
        left->fold_args = ba_camred_args(&d, c->flags);
    } else if (route == CAMRED_SIDE) {
        // (no collective in between at world size 1)
        VLGBA_CHECK(hipEventRecord(d.ev_fork, d.stream));
        VLGBA_CHECK(hipStreamWaitEvent(d.side, d.ev_fork, 0));
        TRY_RC(ba_launch_camera_reduce(&d, c->flags, d.side));
        VLGBA_CHECK(hipEventRecord(d.ev_join, d.side));
        left->side_camred = true;
    } else {
        TRY_RC(ba_launch_camera_reduce(&d, c->flags, d.stream));
    }
    // parity mode: the old SSE again, summed in the reference's flat order
    if (d.parity) TRY_RC(ba_launch_parity_old_sse(&d));
    // U | eA | old_sse travel in one all-reduce (the fast path's reduce
    // kernel writes the old_sse slot itself)
    if (d.ordered)
        VLGBA_CHECK(hipMemcpyAsync(d.eA + d.ld, d.scal + 0, sizeof(double),
                                   hipMemcpyDeviceToDevice, d.stream));
    c->lin_valid = 1;
    c->camred_due = 0;
    return 0;
}

// damping + V*^-1 + Y + Schur complement (S blocks, e_) and their all-reduce;
// left: what this pass's stage 1 handed over (the recovery paths, the getters
// and the covariance: nothing)
int schur_phase(vlgba_ctx *c, double lam, const stage1_left &left)
{
    ba_dev &d = c->d;
    mark(c, 2);
    if (d.ordered) {
        TRY_RC(ba_launch_damp_point(&d, lam));
        mark(c, 3);
        TRY_RC(ba_launch_schur(&d, lam));
    } else {
        mark(c, 3);
        TRY_RC(ba_launch_schur_fast(&d, lam, left.fold ? &left.fold_args : nullptr,
                                 left.side_camred));
    }
    if (c->world > 1 || c->comm) {
        // [S blocks | e_ | old SSE] of this rank's points -> the global system
        double *sse = d.rhs + d.lds;
        VLGBA_CHECK(hipMemcpyAsync(sse, d.eA + d.ld, sizeof(double), hipMemcpyDeviceToDevice,
                                   d.stream));
        TRY_RC(allreduce(c, d.sblk, (size_t)d.na * d.na * d.nb + d.lds + 1));
        VLGBA_CHECK(hipMemcpyAsync(d.scal + 0, sse, sizeof(double), hipMemcpyDeviceToDevice,
                                   d.stream));
    }
    return 0;
}

// the pass scalars after the update: cross-rank sums, then to the host (spin
// on the host-mapped block when single-rank and untimed, else a copy).
// published: the update's final sums already publish them (ba_launch_update)
static int collect_scalars(vlgba_ctx *c, bool spin, bool published, double hs[6])
{
    ba_dev &d = c->d;
    // new SSE, camera and point parts of dp'(lambda dp + g), and the solve's
    // two status words (every rank then takes the same pinv / re-solve
    // decision; scal[0] = the global old SSE, schur_phase)
    if (c->world > 1 || c->comm) TRY_RC(allreduce(c, d.scal + 1, 5));
    if (spin) {
        // spin on the host-mapped sequence number written last (by the update's
        // final sums, or k_publish); lower latency than a copy +
        // hipStreamSynchronize.  A stalled stream falls back to the
        // synchronisation, which reports the error
        if (!published) TRY_RC(ba_launch_publish(&d));
        const double want = (double)d.seq;
        const auto t0 = std::chrono::steady_clock::now();
        bool got = false;
        for (long it = 0;; it++) {
            if (d.hres[7] == want) {
                got = true;
                break;
            }
            if ((it & 1023) == 1023 &&
                std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5))
                break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (got) {
            for (int q = 0; q < 6; q++) hs[q] = d.hres[q];
            return 0;
        }
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
    }
    TRY_RC(download(hs, d.scal, 6, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

// The end the recovery paths share: the update with the da they formed (never
// the one-launch CR's, so k_camera_update runs; nothing publishes), the parity
// sums, the scalars
static int recovery_update(vlgba_ctx *c, double lam, double hs[6])
{
    ba_dev &d = c->d;
    TRY_RC(ba_launch_update(&d, lam, c->flags, false, false, nullptr));
    if (d.parity) TRY_RC(ba_launch_parity_new_sums(&d, lam));
    return collect_scalars(c, false, false, hs);
}

// The reduced solve of a pass, whichever the context has: the block-Jacobi PCG
// on the blocks themselves (it assembles nothing and never forms a_new), or
// the assembly of S and the direct solve the plan chose.  pass: lm_pass's own
// call, which marks the end of the assembly phase (event 5)
static int reduced_solve(vlgba_ctx *c, bool *cam_updated, int nospin, bool pass)
{
    ba_dev &d = c->d;
    *cam_updated = false;
    if (d.pcg) {
        if (pass) mark(c, 5);
        return ba_pcg_solve(&d);
    }
    TRY_RC(ba_launch_assemble(&d));
    if (pass) mark(c, 5);
    return ba_chol_solve(&d, cam_updated, nospin);
}

// A hand-off spin of the one-launch solve gave up (timeout word scal[5]):
// nothing is wrong with S, the launch just did not finish in time.  Re-form
// S and e_ (the solve works in place), solve with the launches that never
// wait on other workgroups, then the same update.  Every rank gets here
// together (the status words travel in the scalars' all-reduce), so the
// collectives of schur_phase pair up.
static int resolve_nospin(vlgba_ctx *c, double lam, double hs[6])
{
    ba_dev &d = c->d;
    TRY_RC(schur_phase(c, lam));
    // (a solve without spins never sets it; a PCG context solves again the same way)
    bool cam_updated = false;
    TRY_RC(reduced_solve(c, &cam_updated, 1, false));
    TRY_RC(recovery_update(c, lam, hs));
    c->spin_retries++;
    if (!d.chol) return 0;
    // one of the envelope runner's own hand-offs gave up (most likely its side
    // stream sharing a hardware queue with the library stream, so the column
    // launches queue behind it): this context's column launches alone from now on
    TRY_RC(std::min(0, ba_env_runner_timed_out(&d)));
    return 0;
}

// dpotrf / dpotri (fn) on the lower triangle of the dense scratch, in place,
// and its info word on the host.  The caller holds g_rs_mu and has set the
// handle's stream.
int rs_factor_info(vlgba_ctx *c, rocblas_handle hdl, decltype(rs_api::potrf) fn, int *info)
{
    const rocblas_int ld = (rocblas_int)c->d.ld;
    if (fn(hdl, rocblas_fill_lower, ld, c->dense.S, ld, c->dense.info) != rocblas_status_success)
        return VLGBA_E_ARG;
    VLGBA_CHECK(hipMemcpyAsync(info, c->dense.info, sizeof *info, hipMemcpyDeviceToHost,
                               c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

// A pass whose nested-dissection Cholesky met a non-positive pivot: the same
// S (the Cholesky took it in place) is assembled densely in the natural
// camera order and factored by rocSOLVER dpotrf before the pinv fallback is
// considered -- the pivot may be an artefact of the elimination order on a
// system whose gauge directions only the damping lifts (cond(S) up to 1e17 on
// the growing replays), and the natural order is the one bundle_euclid.m's
// pinv is then compared with.  Returns 1 if dpotrf fails
// too (the caller takes the pinv step), 0 with the pass finished.
static int nd_natural_retry(vlgba_ctx *c, double lam, double hs[6])
{
    ba_dev &d = c->d;
    rs_api *rs = nullptr;
    rocblas_handle hdl = nullptr;
    TRY_RC(rs_prepare(d.device, &rs, &hdl));
    if (!rs->potrf || !rs->potrs) return 1;
    const long long ld = d.ld;
    TRY_RC(c->dense.ensure(ld));
    TRY_RC(schur_phase(c, lam));
    TRY_RC(ba_launch_assemble_plain(&d, c->dense.S, ld, 1));
    TRY_RC(ba_fix_diag_plain(&d, c->dense.S, ld));   // exactly-zero rows: unit diagonal, rhs 0
    VLGBA_CHECK(hipMemcpyAsync(c->dense.e, d.rhs, sizeof(double) * ld, hipMemcpyDeviceToDevice,
                               d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    int info = 0;
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        if (rs->set_stream(hdl, d.stream) != rocblas_status_success) return VLGBA_E_ARG;
        TRY_RC(rs_factor_info(c, hdl, rs->potrf, &info));
        if (info != 0) return 1;
        if (rs->potrs(hdl, rocblas_fill_lower, (rocblas_int)ld, 1, c->dense.S, (rocblas_int)ld,
                      c->dense.e, (rocblas_int)ld) != rocblas_status_success)
            return VLGBA_E_ARG;
    }
    VLGBA_CHECK(hipMemcpyAsync(d.da, c->dense.e, sizeof(double) * ld, hipMemcpyDeviceToDevice,
                               d.stream));
    TRY_RC(recovery_update(c, lam, hs));
    c->nd_retries++;
    if (c->rank == 0 && !std::getenv("VLGBA_QUIET"))
        std::fprintf(stderr, "[vlgba] non-positive pivot in the nested-dissection order: the "
                             "natural-order Cholesky (dpotrf) took the pass\n");
    return 0;
}

// da = pinv(S) * e_ on the GPU (bundle_euclid.m:193) for a pass whose
// Cholesky met a non-positive pivot: S and e_ again (the solve overwrote them
// in place), the lower triangle of S assembled densely, rocSOLVER dsyevd,
// then V diag(1/ev, |ev| > tol) V^T e_ (ba_pinv_apply), and the update with
// that da.  Every rank runs it on the identical all-reduced system.
static int pinv_fallback(vlgba_ctx *c, double lam, double hs[6])
{
    ba_dev &d = c->d;
    const auto t0 = std::chrono::steady_clock::now();
    rs_api *rs = nullptr;
    rocblas_handle hdl = nullptr;
    TRY_RC(rs_prepare(d.device, &rs, &hdl));
    const long long ld = d.ld;
    TRY_RC(c->dense.ensure(ld));
    TRY_RC(schur_phase(c, lam));
    TRY_RC(ba_launch_assemble_plain(&d, c->dense.S, ld, 1));
    // the library stream is non-blocking: make S complete before rocSOLVER
    // (parts of dsyevd are ordered against the legacy stream, not ours)
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        if (rs->set_stream(hdl, d.stream) != rocblas_status_success ||
            rs->syevd(hdl, rocblas_evect_original, rocblas_fill_lower, (rocblas_int)ld,
                      c->dense.S, (rocblas_int)ld, c->dense.ev, c->dense.e,
                      c->dense.info) != rocblas_status_success)
            return VLGBA_E_ARG;
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
    }
    {
        int info = 0;
        VLGBA_CHECK(hipMemcpy(&info, c->dense.info, sizeof info, hipMemcpyDeviceToHost));
        if (info != 0) return VLGBA_E_ARG;   // the eigensolver did not converge
    }
    TRY_RC(ba_pinv_apply(&d, c->dense.S, c->dense.ev, ld, d.rhs, c->dense.w, d.da));
    TRY_RC(recovery_update(c, lam, hs));
    c->pinv_used++;
    if (c->rank == 0 && !std::getenv("VLGBA_QUIET"))
        std::fprintf(stderr,
                     "[vlgba] non-positive pivot: da = pinv(S) e_ by dsyevd on the dense "
                     "%lld x %lld S (%.1f MB of device memory), %.3f s\n",
                     ld, ld, 8e-6 * (double)ld * (double)ld,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

static int lm_pass(vlgba_ctx *c, int relinearize, vlgba_step_info *info)
{
    ba_dev &d = c->d;
    const double lam = c->lambda;
    mark(c, 0);
    // U / eA / old SSE of a relinearised pass: workgroups of this pass's MFMA
    // Schur launch when the plan has MFMA groups; else, single-rank and
    // untimed, on the side stream (ba_launch_schur_fast joins before
    // k_schur_reduce); else a launch of their own
    const camred_route route = !d.ordered && d.ngrp_mf > 0 ? CAMRED_FOLD
                               : !d.ordered && c->world == 1 && !c->timing ? CAMRED_SIDE
                                                                           : CAMRED_PLAIN;
    stage1_left left;
    TRY_RC(stage1(c, relinearize, route, &left));
    TRY_RC(schur_phase(c, lam, left));
    mark(c, 4);
    bool cam_updated = false;   // the solve formed a_new / rot_new (one-launch CR)
    TRY_RC(reduced_solve(c, &cam_updated, 0, true));
    for (int w = 4; w <= 5; w++) {   // test hooks: as if a pivot failed / a spin gave up
        int &k = w == 4 ? c->debug_pivots : c->debug_timeouts;
        if (k > 0) {
            static const double one = 1.0;
            VLGBA_CHECK(hipMemcpyAsync(d.scal + w, &one, sizeof one, hipMemcpyHostToDevice,
                                       d.stream));
            k--;
        }
    }
    mark(c, 6);
    // RCCL ranks spin as well: their collectives are stream-ordered, and the
    // publish then follows the scalars' all-reduce (collect_scalars)
    const bool spin = (c->world == 1 || c->comm) && !c->timing;
    // (without RCCL the fast update's final-sums launch publishes)
    bool published = false;
    TRY_RC(ba_launch_update(&d, lam, c->flags, cam_updated, spin && !c->comm, &published));
    if (d.parity) TRY_RC(ba_launch_parity_new_sums(&d, lam));
    mark(c, 7);
    // scalars: [0] old_sse [1] new_sse [2] dpg cameras [3] dpg points
    // [4] non-positive pivot [5] hand-off spin timeout (summed over ranks)
    double hs[6];
    TRY_RC(collect_scalars(c, spin, published, hs));
    info->pinv = 0;
    info->spin_retry = 0;
    info->nd_retry = 0;
    if (hs[5] != 0.0) {   // the solve did not finish: again, without spins
        TRY_RC(resolve_nospin(c, lam, hs));
        info->spin_retry = 1;
    }
    // the nested-dissection order's pivot: the natural order first
    if (hs[4] != 0.0 && d.chol && d.chol->plan.nd_np > 0) {
        const int rc = nd_natural_retry(c, lam, hs);
        if (rc < 0) return rc;
        info->nd_retry = 1;
        if (rc == 0) hs[4] = 0.0;
    }
    if (hs[4] != 0.0) {
        // non-positive pivot: bundle_euclid.m:193 takes pinv(S)*e_ whatever S is
        // (App. A Q8), so does the fallback -- then the same update
        TRY_RC(pinv_fallback(c, lam, hs));
        info->pinv = 1;
    }
    if (c->timing) {
        float ms;
        const int map[7][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}};
        for (int q = 0; q < 7; q++) {
            (void)hipEventElapsedTime(&ms, c->ev[map[q][0]], c->ev[map[q][1]]);
            c->phase_ms[q] = ms;
        }
        ba_ktimer *kt = d.kt;
        for (int q = 0; kt && q + 1 < kt->nev; q += 2) {
            (void)hipEventElapsedTime(&ms, kt->ev[q], kt->ev[q + 1]);
            kt->ms[kt->kid[q / 2]] += ms;
            kt->calls[kt->kid[q / 2]]++;
        }
        if (kt) kt->nev = 0;
        if (kt && d.chol) {
            // the solve's algorithmic flops (chol_plan_build's count) on the timers
            // that ran them: one-launch / per-level CR, or the envelope's steps,
            // separator SYRK and backward solve
            const chol_plan &P = d.chol->plan;
            const bool cr = P.cr_nlev > 0;
            kt->flops[cr ? KT_CR_FACTOR : KT_FACTOR] += P.fl_factor;
            kt->flops[KT_SYRK] += P.fl_syrk;
            kt->flops[cr ? KT_CR_BACK : KT_BACKWARD] += P.fl_back;
        }
    }
    info->old_sse = hs[0];
    info->new_sse = hs[1];
    info->dpg = hs[2] + hs[3];
    info->lambda = lam;
    info->chol_failed = info->pinv;   // the Cholesky failed; the step is pinv(S)*e_
    info->rho = (hs[0] - hs[1]) / info->dpg;
    if (c->model == VLGBA_MODEL_PROJECTIVE)   // bundle_projective.m:182-188 (normalised first)
        info->accepted = 1 / c->num_vis * hs[1] < 1 / c->num_vis * hs[0];
    else                                      // bundle_euclid.m:218
        info->accepted = (hs[0] - hs[1]) > 0;
    return 0;
}

// bundle_euclid.m:218-241 (bundle_projective.m:188-207) applied to the context
static void lm_apply(vlgba_ctx *c, const vlgba_step_info *info)
{
    ba_dev &d = c->d;
    const bool proj = c->model == VLGBA_MODEL_PROJECTIVE;
    if (info->accepted) {
        std::swap(d.a, d.a_new);
        std::swap(d.b, d.b_new);
        std::swap(d.rot, d.rot_new);   // rotation table of the new a
        if (d.fused) {   // the update linearised at the new point: take it
            std::swap(d.W, d.W2);
            std::swap(d.V, d.V2);
            std::swap(d.eB, d.eB2);
            std::swap(d.upart, d.upart2);
            std::swap(d.chsse, d.chsse2);
        }
        if (proj)
            c->lambda = c->lambda / 10;
        else
            c->lambda = c->lambda * std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * info->rho - 1.0, 3));
        c->nu = 2.0;
        c->lin_valid = d.fused ? 1 : 0;
        c->camred_due = d.fused ? 1 : 0;
    } else if (proj) {
        c->lambda = c->lambda * 10;
    } else {
        c->lambda = c->lambda * c->nu;
        c->nu = 2.0 * c->nu;
    }
}

// device rows of k doubles in the internal order -> host, row i to row perm[i]
// of the input order (perm empty: the same order; else synchronous)
static int download_rows(vlgba_ctx *c, double *dst, const double *src, size_t k, size_t rows,
                         const std::vector<int> &perm)
{
    if (perm.empty()) return download(dst, src, k * rows, c->d.stream);
    std::vector<double> tmp(k * rows);
    TRY_RC(download(tmp.data(), src, k * rows, c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    for (size_t i = 0; i < rows; i++)
        std::memcpy(dst + k * perm[i], tmp.data() + k * i, sizeof(double) * k);
    return 0;
}

int download_points(vlgba_ctx *c, double *dst, const double *src, int k)
{
    return download_rows(c, dst, src, (size_t)k, (size_t)c->d.n, c->pperm);
}

// =========================================================================
// C ABI
// =========================================================================
extern "C" {

int vlgba_version(char *buf, int len)
{
    const int n = (int)std::strlen(VLGBA_VERSION_STR);
    if (buf && len > 0) {
        std::strncpy(buf, VLGBA_VERSION_STR, (size_t)len - 1);
        buf[len - 1] = 0;
    }
    return n;
}

int vlgba_abi_check(int abi_version, long long sz_problem, long long sz_options,
                    long long sz_stats, long long sz_step_info, long long sz_resect_problem)
{
    const bool ok = abi_version == VLGBA_ABI_VERSION &&
                    sz_problem == (long long)sizeof(vlgba_problem) &&
                    sz_options == (long long)sizeof(vlgba_options) &&
                    sz_stats == (long long)sizeof(vlgba_stats) &&
                    sz_step_info == (long long)sizeof(vlgba_step_info) &&
                    sz_resect_problem == (long long)sizeof(vlgba_resect_problem);
    return ok ? 0 : VLGBA_E_ABI;
}

int vlgba_get_unique_id(void *id128)
{
    if (!id128) return VLGBA_E_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return VLGBA_E_COMM;
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof id);
    return 0;
}

int vlgba_comm_release(const void *id128)
{
    return id128 ? comm_forget(id128) : VLGBA_E_ARG;
}

int vlgba_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vlgba_create(const vlgba_problem *prob, const vlgba_options *opt, vlgba_ctx **out)
{
    if (!out) return VLGBA_E_ARG;
    return ctx_create(prob, opt, out, true, true, false);
}

void vlgba_destroy(vlgba_ctx *ctx)
{
    if (ctx) (void)ctx_enter(ctx);
    ctx_free(ctx);
}

int vlgba_set_params(vlgba_ctx *c, const double *a, const double *b)
{
    if (!c || !a || !b) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    static const bool pageable = std::getenv("VLGBA_SETP_PAGEABLE") != nullptr;   // A/B
    const size_t na = (size_t)c->d.ld, nb = 3 * (size_t)c->d.n;
    // pinned staging: the copies start at once
    double *ha = pageable ? nullptr : aux_pin(c->aux, na + nb), *hb = ha ? ha + na : nullptr;
    if (ha) std::memcpy(ha, a, sizeof(double) * na);
    TRY_RC(upload(c->d.a, ha ? ha : a, na, c->d.stream));
    if (!c->pperm.empty()) {   // input point order -> internal order
        double *dst = hb;
        if (!dst) {
            c->hb_tmp.resize(nb);
            dst = c->hb_tmp.data();
        }
        for (int i = 0; i < c->d.n; i++)
            for (int r = 0; r < 3; r++)
                dst[3 * (size_t)i + r] = b[3 * ((size_t)c->p0 + c->pperm[i]) + r];
        TRY_RC(upload(c->d.b, dst, nb, c->d.stream));
    } else if (hb) {
        std::memcpy(hb, b + 3 * (size_t)c->p0, sizeof(double) * nb);
        TRY_RC(upload(c->d.b, hb, nb, c->d.stream));
    } else {
        TRY_RC(upload(c->d.b, b + 3 * (size_t)c->p0, nb, c->d.stream));
    }
    TRY_RC(ba_launch_rotations(&c->d, c->d.a, c->d.rot));
    c->lin_valid = 0;
    static const bool tm = std::getenv("VLGBA_SETP_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    if (tm)
        std::fprintf(stderr, "[vlgba set_params] m=%d sync %.3f ms\n", c->d.m,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                         .count());
    return 0;
}

int vlgba_get_params(vlgba_ctx *c, double *a, double *b)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    if (a) TRY_RC(download(a, c->d.a, (size_t)c->d.ld, c->d.stream));
    if (b) {
        if (c->world > 1) {
            // every rank returns the full b: all-reduce of a zero-padded copy
            ba_dtmp<double> full(c->d.stream);
            TRY_RC(full.alloc(3 * (size_t)c->n_global));
            VLGBA_CHECK(hipMemsetAsync(full, 0, sizeof(double) * 3 * c->n_global, c->d.stream));
            if (c->pperm.empty()) {
                VLGBA_CHECK(hipMemcpyAsync(full + 3 * (size_t)c->p0, c->d.b,
                                           sizeof(double) * 3 * c->d.n, hipMemcpyDeviceToDevice,
                                           c->d.stream));
            } else {   // internal -> input order inside this rank's range
                c->hb_tmp.resize(3 * (size_t)c->d.n);
                TRY_RC(download_points(c, c->hb_tmp.data(), c->d.b, 3));
                VLGBA_CHECK(hipMemcpyAsync(full + 3 * (size_t)c->p0, c->hb_tmp.data(),
                                           sizeof(double) * 3 * c->d.n, hipMemcpyHostToDevice,
                                           c->d.stream));
                VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
            }
            TRY_RC(allreduce(c, full, 3 * (size_t)c->n_global));
            TRY_RC(download(b, full.get(), 3 * (size_t)c->n_global, c->d.stream));
        } else {
            TRY_RC(download_points(c, b, c->d.b, 3));
        }
    }
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

// U / eA stay per-rank partials on the device (schur_owner); the caller gets
// their sum over ranks
static int download_camera_sums(vlgba_ctx *c, double *U, double *eA)
{
    ba_dev &d = c->d;
    const size_t nu = (size_t)d.na * d.na * d.m, nue = nu + d.ld + 1;
    ba_dtmp<double> sum(d.stream);
    const double *ue = d.U;
    if (c->world > 1) {
        TRY_RC(sum.alloc(nue));
        VLGBA_CHECK(hipMemcpyAsync(sum, d.U, sizeof(double) * nue, hipMemcpyDeviceToDevice,
                                   d.stream));
        TRY_RC(allreduce(c, sum, nue));
        ue = sum;
    }
    if (U) TRY_RC(download(U, ue, nu, d.stream));
    if (eA) TRY_RC(download(eA, ue + nu, (size_t)d.ld, d.stream));
    return 0;
}

int vlgba_get_linearization(vlgba_ctx *c, double *U, double *eA, double *V, double *eB,
                            double *W)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    ba_dev &d = c->d;
    // the linearisation the context holds for the current parameters (a
    // rejected step's, or the one the fused update made at an accepted step's
    // new point), else a new one
    TRY_RC(stage1(c, 0, CAMRED_PLAIN, nullptr));
    TRY_RC(download_camera_sums(c, U, eA));
    if (V) TRY_RC(download_points(c, V, d.V, 9));
    if (eB) TRY_RC(download_points(c, eB, d.eB, 3));
    if (W) TRY_RC(download_rows(c, W, d.W, (size_t)3 * d.na, (size_t)d.N, c->operm));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

int vlgba_get_reduced_system(vlgba_ctx *c, int *blk_jk, double *blocks, double *e_)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    ba_dev &d = c->d;
    TRY_RC(stage1(c, 0, CAMRED_PLAIN, nullptr));
    TRY_RC(schur_phase(c, c->lambda));
    if (blk_jk) TRY_RC(download(blk_jk, d.blk_jk, 2 * (size_t)d.nb, d.stream));
    if (blocks) TRY_RC(download(blocks, d.sblk, (size_t)d.na * d.na * d.nb, d.stream));
    if (e_) TRY_RC(download(e_, d.rhs, (size_t)d.ld, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

int vlgba_set_loss(vlgba_ctx *c, int kind, double scale)
{
    if (!c || kind < VLGBA_LOSS_NONE || kind > VLGBA_LOSS_CAUCHY) return VLGBA_E_ARG;
    if (kind != VLGBA_LOSS_NONE && !(std::isfinite(scale) && scale > 0)) return VLGBA_E_ARG;
    // ordered / parity mode exists for bit parity with a reference that has no loss
    if (c->d.ordered) return VLGBA_E_ARG;
    c->d.loss_kind = kind;
    c->d.loss_scale = kind != VLGBA_LOSS_NONE ? scale : 0.0;
    c->lin_valid = 0;   // the next pass / getter linearises with the new weights
    return 0;
}

int vlgba_set_jacobian(vlgba_ctx *c, int kind)
{
    if (!c || (kind != VLGBA_JAC_FD && kind != VLGBA_JAC_ANALYTIC)) return VLGBA_E_ARG;
    // ordered / parity mode exists for bit parity with the reference's differences
    if (c->d.ordered) return VLGBA_E_ARG;
    // the radial model has the closed form only
    if (c->d.na == BA_RAD_NA && kind != VLGBA_JAC_ANALYTIC) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    c->d.jac = kind;
    // the table of the current a in the new mode's layout; a camera update the
    // last solve folded in built the other one
    TRY_RC(ba_launch_rotations(&c->d, c->d.a, c->d.rot));
    c->lin_valid = 0;
    return 0;
}

int vlgba_get_jacobian(vlgba_ctx *c, int *kind)
{
    if (!c) return VLGBA_E_ARG;
    if (kind) *kind = c->d.jac;
    return 0;
}

int vlgba_get_loss(vlgba_ctx *c, int *kind, double *scale)
{
    if (!c) return VLGBA_E_ARG;
    if (kind) *kind = c->d.loss_kind;
    if (scale) *scale = c->d.loss_scale;
    return 0;
}

int vlgba_get_residuals(vlgba_ctx *c, double *e, double *w, double *rho)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    ba_dev &d = c->d;
    const size_t N = (size_t)d.N;
    if (N == 0 || (!e && !w && !rho)) return 0;
    ba_dtmp<double> buf(d.stream);   // e [N][2] | w [N] | rho [N], internal observation order
    TRY_RC(buf.alloc(4 * N));
    // the rotation table of d.a is current (set_params / an accepted step)
    TRY_RC(ba_launch_obs_residuals(&d, e ? buf.get() : nullptr, w ? buf + 2 * N : nullptr,
                                   rho ? buf + 3 * N : nullptr));
    double *dst[3] = {e, w, rho};
    const size_t off[3] = {0, 2 * N, 3 * N}, wd[3] = {2, 1, 1};
    for (int q = 0; q < 3; q++)
        if (dst[q]) TRY_RC(download_rows(c, dst[q], buf + off[q], wd[q], N, c->operm));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

int vlgba_get_step(vlgba_ctx *c, double *da, double *db)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    if (da) TRY_RC(download(da, c->d.da, (size_t)c->d.ld, c->d.stream));
    if (db) TRY_RC(download_points(c, db, c->d.db, 3));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

int vlgba_debug_force_status(vlgba_ctx *c, int word, int passes)
{
    if (!c || word < 4 || word > 6 || passes < 0) return VLGBA_E_ARG;
    if (word == 6) {
        if (c->d.chol) c->d.chol->debug_runner_fail = passes;
    } else
        (word == 4 ? c->debug_pivots : c->debug_timeouts) = passes;
    return 0;
}

int vlgba_set_pcg(vlgba_ctx *c, double tol, int max_iter)
{
    if (!c || !c->d.pcg || !std::isfinite(tol) || tol >= 1.0) return VLGBA_E_ARG;
    if (tol > 0.0) c->d.pcg->tol = tol;
    if (max_iter > 0) c->d.pcg->max_iter = max_iter;
    return 0;
}

int vlgba_get_pcg(vlgba_ctx *c, double *tol, int *max_iter)
{
    if (!c || !c->d.pcg) return VLGBA_E_ARG;
    if (tol) *tol = c->d.pcg->tol;
    if (max_iter) *max_iter = c->d.pcg->max_iter;
    return 0;
}

int vlgba_get_pcg_stats(vlgba_ctx *c, int *iterations, double *relres, int *converged,
                        long long *total)
{
    if (!c || !c->d.pcg) return VLGBA_E_ARG;
    const ba_pcg &P = *c->d.pcg;
    if (iterations) *iterations = P.iters;
    if (relres) *relres = P.relres;
    if (converged) *converged = P.conv;
    if (total) *total = P.total;
    return 0;
}

int vlgba_set_timing(vlgba_ctx *c, int on)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    if (on && !c->ev[0]) {   // all eight events or none
        hipEvent_t ev[8] = {};
        hipError_t err = hipSuccess;
        for (int q = 0; q < 8 && err == hipSuccess; q++) err = hipEventCreate(&ev[q]);
        if (err != hipSuccess) {
            for (auto &e : ev)
                if (e) (void)hipEventDestroy(e);
            return -(int)err;
        }
        std::memcpy(c->ev, ev, sizeof ev);
    }
    if (on && !c->d.kt) {
        c->d.kt = new (std::nothrow) ba_ktimer();
        if (!c->d.kt) return VLGBA_E_NOMEM;
    }
    c->timing = on;
    if (c->d.kt) c->d.kt->on = on;
    return 0;
}

int vlgba_kernel_ms(vlgba_ctx *c, double *ms, long long *calls, int reset)
{
    if (!c) {   // process-wide: the destroyed contexts' timers
        kt_totals(ms, calls, nullptr, reset);
        return 0;
    }
    if (!c->d.kt) return VLGBA_E_ARG;
    for (int k = 0; k < KT_N; k++) {
        if (ms) ms[k] = c->d.kt->ms[k];
        if (calls) calls[k] = c->d.kt->calls[k];
        if (reset) {
            c->d.kt->ms[k] = 0.0;
            c->d.kt->calls[k] = 0;
            c->d.kt->flops[k] = 0.0;
        }
    }
    return 0;
}

int vlgba_kernel_flops(vlgba_ctx *c, double *flops)
{
    if (!flops) return VLGBA_E_ARG;
    if (!c) {
        kt_totals(nullptr, nullptr, flops, 0);
        return 0;
    }
    if (!c->d.kt) return VLGBA_E_ARG;
    for (int k = 0; k < KT_N; k++) flops[k] = c->d.kt->flops[k];
    return 0;
}

const char *vlgba_kernel_name(int k)
{
    static const char *names[KT_N] = {
        "k_rotations", "k_linearize", "k_camera_reduce", "k_damp_point", "k_schur",
        "k_schur_group", "k_schur_reduce", "k_assemble", "k_factor_step", "k_syrk",
        "k_backward", "k_camera_update", "k_point_update", "k_cr_factor", "k_cr_update",
        "k_cr_back", "k_schur_mfma", "k_update_linearize"};
    return (k >= 0 && k < KT_N) ? names[k] : "";
}

int vlgba_plan_info(vlgba_ctx *c, long long *info, int len)
{
    if (!c || !info) return VLGBA_E_ARG;
    const ba_dev &d = c->d;
    // the solve's slots: zeros in a stage-mode context (no solve, no plan)
    static const chol_plan no_plan;
    const chol_plan &P = d.chol ? d.chol->plan : no_plan;
    const long long ne = P.cr_nlev ? P.eptr[P.cr_nlev] : 0;
    const long long nk = P.cr_nlev ? P.kptr[P.cr_nlev] : 0;
    const long long v[VLGBA_NPLAN] = {d.N,   d.n,    d.m,   d.na,         d.nch,  d.ns,
                                      d.nes, d.ngrp, d.ngs, d.nge,        d.nb,   P.nt,
                                      P.cr_nlev, ne, nk,    d.ordered,    d.ordered ? d.T : d.nterm_fast,
                                      d.blob_words, d.mfma,
                                      P.cr_nlev ? (P.cr32 ? P.tb32 : 64) : 0,
                                      d.ngrp_mf, c->pperm.empty() ? 0 : 1, d.nl, P.nd_np,
                                      P.nd_np ? P.nt - P.nd_a0[P.nd_np] : 0,
                                      (long long)P.fl_factor, (long long)P.fl_syrk,
                                      (long long)P.fl_back, d.chol ? d.chol->runner_runs : 0,
                                      d.vinv_fold, d.camupd_fold, d.pcg ? 1 : 0,
                                      d.pcg ? d.pcg->bytes : d.chol ? d.chol->bytes : 0};
    for (int k = 0; k < len && k < VLGBA_NPLAN; k++) info[k] = v[k];
    return VLGBA_NPLAN;
}

int vlgba_phase_ms(vlgba_ctx *c, double *ms7)
{
    if (!c || !ms7) return VLGBA_E_ARG;
    for (int q = 0; q < 7; q++) ms7[q] = c->phase_ms[q];
    return 0;
}

int vlgba_sync(vlgba_ctx *c)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

int vlgba_step(vlgba_ctx *c, int relinearize, int update_lm, vlgba_step_info *info)
{
    if (!c) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    vlgba_step_info tmp;
    if (!info) info = &tmp;
    TRY_RC(lm_pass(c, relinearize, info));
    if (update_lm) lm_apply(c, info);
    return 0;
}

int vlgba_run_passes(vlgba_ctx *c, int npass, vlgba_step_info *info)
{
    if (!c || npass < 0) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    vlgba_step_info tmp;
    if (!info) info = &tmp;
    std::memset(info, 0, sizeof *info);
    for (int q = 0; q < npass; q++) TRY_RC(lm_pass(c, 1, info));
    return 0;
}

// bundle_euclid.m:111-249
int vlgba_run(vlgba_ctx *c, double *error_out, int error_cap, vlgba_stats *stats)
{
    if (!c || (error_out && error_cap < 0)) return VLGBA_E_ARG;
    TRY_RC(ctx_enter(c));
    auto t0 = std::chrono::steady_clock::now();
    c->lambda = c->lambda0;
    c->nu = 2.0;
    c->lin_valid = 0;
    std::vector<double> err;   // error_, 1-based in the reference
    int iter = 1, iter2 = 0, passes = 0, acc = 0;
    const int pinv0 = c->pinv_used, retry0 = c->spin_retries, nd0 = c->nd_retries;
    for (;;) {
        if (!(iter < c->max_iter && iter2 < c->max_iter2)) break;
        if (iter >= 3) {
            const double e1 = err[iter - 1], e0 = err[iter - 2];
            if (!(e1 > 1e-20 && e0 - e1 > c->stop_rel * e0)) break;
        }
        vlgba_step_info info;
        TRY_RC(lm_pass(c, 0, &info));
        passes++;
        if (info.accepted) {
            const bool proj = c->model == VLGBA_MODEL_PROJECTIVE;
            // bundle_euclid.m:219-220 divide; bundle_projective.m:182-183 scale by 1/num_vis
            const double olde = proj ? 1 / c->num_vis * info.old_sse : info.old_sse / c->num_vis;
            const double newe = proj ? 1 / c->num_vis * info.new_sse : info.new_sse / c->num_vis;
            if (c->verbose && c->rank == 0)
                std::printf("iter %d: error= %.5g -> %.5g\n", iter, olde, newe);
            if ((int)err.size() < iter) err.push_back(olde);
            else err[iter - 1] = olde;
            iter++;
            err.push_back(newe);
            iter2 = 0;
            acc++;
        } else {
            iter2++;
        }
        lm_apply(c, &info);
        if (c->on_pass && c->rank == 0) c->on_pass(passes, iter, &info, c->on_pass_user);
    }
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    if (error_out)   // at most error_cap entries; stats->num_error is the full count
        for (size_t q = 0; q < err.size() && q < (size_t)error_cap; q++) error_out[q] = err[q];
    if (stats) {
        stats->iterations = passes;
        stats->accepted = acc;
        stats->num_error = (int)err.size();
        stats->lambda = c->lambda;
        stats->pinv_passes = c->pinv_used - pinv0;
        stats->spin_retries = c->spin_retries - retry0;
        stats->nd_retries = c->nd_retries - nd0;
        stats->seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

int vlgba_solve(const vlgba_problem *prob, const vlgba_options *opt, double *a, double *b,
                double *error_out, int error_cap, vlgba_stats *stats)
{
    if (!a || !b) return VLGBA_E_ARG;
    vlgba_ctx *c = nullptr;
    TRY_RC(vlgba_create(prob, opt, &c));
    const ctx_ptr owner(c);
    TRY_RC(vlgba_set_params(c, a, b));
    TRY_RC(vlgba_run(c, error_out, error_cap, stats));
    return vlgba_get_params(c, a, b);
}

}  // extern "C"
