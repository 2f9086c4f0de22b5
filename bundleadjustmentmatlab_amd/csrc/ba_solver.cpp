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
#include "ba_internal.h"
#include "ba_plan.h"   // the host planner: sort_obs, order_points_by_kind, plan_host
#include "ba_chol.h"   // the reduced solve's state and plan (ba_dev::chol)
#include "ba_pcg.h"    // ... or the block-Jacobi PCG's (ba_dev::pcg)
#include "../../include/vlgba.h"

#include <rccl/rccl.h>
#include <rocsolver/rocsolver.h>   // types only: the library is dlopen'ed on first use

#include <dlfcn.h>
#include <cstdlib>
#include <string>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <map>
#include <new>
#include <numeric>
#include <vector>

#define VLGBA_STR2(x) #x
#define VLGBA_STR(x) VLGBA_STR2(x)
#define VLGBA_VERSION_STR \
    "vlgba 0.2 (abi " VLGBA_STR(VLGBA_ABI_VERSION) ", gfx950, fp64, MFMA-f64 Cholesky)"

// ---------------------------------------------------------------------------
// Device memory: a per-device caching allocator.  A solve's context makes a few
// dozen allocations; hipMalloc / hipFree of each costs tens of microseconds,
// which the growing-BA replay (hundreds of small solves) would pay every time.
// Blocks are rounded up to a power of two (256 B .. 1 GiB) and kept on a free
// list when released; larger blocks go straight back to HIP.
// ---------------------------------------------------------------------------
namespace {
std::mutex g_mem_mu;
std::multimap<std::pair<int, size_t>, void *> g_mem_free;     // (device, bucket) -> block
std::unordered_map<void *, std::pair<int, size_t>> g_mem_live;  // block -> (device, bucket)
constexpr size_t BA_MEM_CACHE_MAX = size_t(1) << 30;

size_t mem_bucket(size_t bytes)
{
    if (bytes > BA_MEM_CACHE_MAX) return bytes;
    size_t b = 256;
    while (b < bytes) b <<= 1;
    return b;
}
}   // namespace

// VLGBA_POISON=1 (debugging): every block handed out is filled with 0xff
// bytes (NaN doubles, -1 ints), so a kernel that reads memory it never wrote
// shows up as NaN instead of as a stale value of a previous context
static void *poisoned(void *p, size_t b)
{
    static const bool on = std::getenv("VLGBA_POISON") != nullptr;
    if (on && p) {   // null-stream memset: not ordered with non-blocking streams
        (void)hipMemset(p, 0xff, b);
        (void)hipDeviceSynchronize();
    }
    return p;
}

void *ba_dmalloc(size_t bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const size_t b = mem_bucket(bytes ? bytes : 1);
    {
        std::lock_guard<std::mutex> lk(g_mem_mu);
        auto it = g_mem_free.find({dev, b});
        if (it != g_mem_free.end()) {
            void *p = it->second;
            g_mem_free.erase(it);
            g_mem_live[p] = {dev, b};
            return poisoned(p, b);
        }
    }
    void *p = nullptr;
    if (hipMalloc(&p, b) != hipSuccess) {
        // out of memory with blocks cached: give them back and retry once
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> lk(g_mem_mu);
            for (auto &kv : g_mem_free) drop.push_back(kv.second);
            g_mem_free.clear();
        }
        for (void *q : drop) (void)hipFree(q);
        if (hipMalloc(&p, b) != hipSuccess) return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_mem_mu);
    g_mem_live[p] = {dev, b};
    return poisoned(p, b);
}

void ba_dfree(void *p)
{
    if (!p) return;
    std::unique_lock<std::mutex> lk(g_mem_mu);
    auto it = g_mem_live.find(p);
    if (it == g_mem_live.end()) {   // not ours
        lk.unlock();
        (void)hipFree(p);
        return;
    }
    const auto key = it->second;
    g_mem_live.erase(it);
    if (key.second > BA_MEM_CACHE_MAX) {
        lk.unlock();
        (void)hipFree(p);
        return;
    }
    g_mem_free.emplace(key, p);
}

int ba_ensure_dyn_lds(const void *fn, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> done;
    int dev = 0;
    VLGBA_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    size_t &have = done[{fn, dev}];
    if (bytes > have) {
        VLGBA_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)bytes));
        have = bytes;
    }
    return 0;
}

namespace {

// dalloc, upload, download: ba_internal.h
#define TRY(x)                                                                     \
    do {                                                                            \
        int rc__ = (x);                                                             \
        if (rc__) return rc__;                                                      \
    } while (0)

}  // namespace

void kt_begin(ba_ktimer *t, hipStream_t s)
{
    if (t->nev + 2 > KT_MAX_EV) return;
    while (t->ncreated < t->nev + 2) {
        if (hipEventCreate(&t->ev[t->ncreated]) != hipSuccess) return;   // (kt_end skips too)
        t->ncreated++;
    }
    (void)hipEventRecord(t->ev[t->nev], s);
}

void kt_end(ba_ktimer *t, hipStream_t s, int kid)
{
    if (t->nev + 2 > KT_MAX_EV || t->nev + 2 > t->ncreated) return;
    (void)hipEventRecord(t->ev[t->nev + 1], s);
    t->kid[t->nev / 2] = kid;
    t->nev += 2;
}

// =========================================================================
struct ba_aux {
    int device;
    hipStream_t stream, side;
    hipEvent_t ev_fork, ev_join;
    double *hres_host, *hres_dev;
    double *pin;        // pinned host staging of set_params (grown on demand)
    size_t pin_cap;     // its capacity in doubles
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
    hipEvent_t ev[8] = {};
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
    // pinv fallback of the reduced solve (allocated on first use)
    double *pinv_S = nullptr, *pinv_ev = nullptr, *pinv_e = nullptr, *pinv_w = nullptr;
    int *pinv_info = nullptr;
    int pinv_used = 0;            // passes that took the pinv fallback
    int nd_retries = 0;           // nested-dissection pivots solved in the natural order
    int spin_retries = 0;         // passes re-solved after a hand-off timeout
    int debug_timeouts = 0;       // test hooks: passes whose timeout word / pivot word
    int debug_pivots = 0;         // is forced (vlgba_debug_force_status)
    // vlgba_covariance (allocated on its first call): the points binned by track
    // length for k_point_cov (internal order: 8 lanes | one wave | one workgroup
    // per point), the longest track, the points with an observation, the
    // fixed-row mask of S0, the diagonal blocks of Sigma_a and Sigma_b
    int *cov_list = nullptr;
    int cov_n8 = 0, cov_n64 = 0, cov_nwg = 0, cov_tmax = 0, cov_seen = 0;
    unsigned char *cov_fixed = nullptr;
    double *cov_diag = nullptr, *cov_pts = nullptr;
    // ... and the packed copy of Sigma_a's co-visible blocks k_point_cov reads
    // (CSR by camera row: cov_rowptr [m + 1], cov_col / cov_bj [nb];
    // VLGBA_COV_PACKED=0: the dense method's kernel reads the dense inverse -- A/B)
    int *cov_rowptr = nullptr, *cov_col = nullptr, *cov_bj = nullptr;
    double *cov_packed = nullptr;
    int cov_src_packed = 1;       // k_point_cov of the dense method reads the packed copy
    std::vector<int> cov_ord;     // packed block p is block cov_ord[p] of blk_jk
    // the last successful call's blocks are in cov_packed (times cov_scale:
    // vlgba_get_covariance_blocks)
    int cov_have = 0;
    double cov_scale = 1.0;
    // VLGBA_COV_SELECTED (vlgba_set_covariance_method): the selected inverse on
    // the camera-aligned CR factors -- its tile sources and three 32 x 32 tiles
    // per CR tile (allocated on the method's first call)
    int cov_method = VLGBA_COV_DENSE;
    int *cov_selsrc = nullptr;
    double *cov_sig = nullptr;
};

// Per-device pool of the context's streams, fork/join events and host-mapped
// result block: creating them (pinned host memory above all) costs ~0.4 ms,
// which the growing-BA replay would pay per solve.  A context takes one set
// for its lifetime and returns it idle (both streams synchronised).
static std::mutex g_aux_mu;
static std::vector<ba_aux> g_aux_pool;

static int aux_acquire(int device, ba_aux &a)
{
    {
        std::lock_guard<std::mutex> lk(g_aux_mu);
        for (size_t q = 0; q < g_aux_pool.size(); q++)
            if (g_aux_pool[q].device == device) {
                a = g_aux_pool[q];
                g_aux_pool.erase(g_aux_pool.begin() + (long)q);
                a.hres_host[7] = 0.0;   // sequence numbers restart at 1
                return 0;
            }
    }
    std::memset(&a, 0, sizeof a);
    a.device = device;
    void *h = nullptr;
    if (hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&a.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&a.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&a.ev_join, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&h, 8 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer((void **)&a.hres_dev, h, 0) != hipSuccess) {
        if (a.stream) (void)hipStreamDestroy(a.stream);
        if (a.side) (void)hipStreamDestroy(a.side);
        if (a.ev_fork) (void)hipEventDestroy(a.ev_fork);
        if (a.ev_join) (void)hipEventDestroy(a.ev_join);
        if (h) (void)hipHostFree(h);
        return -1;
    }
    std::memset(h, 0, 8 * sizeof(double));
    a.hres_host = (double *)h;
    return 0;
}

static void aux_release(const ba_aux &a)
{
    (void)hipStreamSynchronize(a.stream);
    (void)hipStreamSynchronize(a.side);
    std::lock_guard<std::mutex> lk(g_aux_mu);
    g_aux_pool.push_back(a);
}

// RCCL communicators outlive their context, keyed by (unique id, world size,
// rank): a caller that passes the same id again (dist.run_sharded keeps one
// id per device set for a whole growing replay) takes the idle communicator
// instead of paying ncclCommInitRank per solve.  One context per key at a
// time.  An idle communicator is destroyed only when its caller says the id
// is done (vlgba_comm_release): a unique id serves ONE bootstrap, so evicting
// the communicator of an id the caller may pass again would send that next
// context into an ncclCommInitRank that waits forever.
struct comm_key {
    std::string id;
    int world, rank;
    bool operator<(const comm_key &o) const
    {
        if (id != o.id) return id < o.id;
        if (world != o.world) return world < o.world;
        return rank < o.rank;
    }
};
static std::mutex g_comm_mu;
static std::multimap<comm_key, ncclComm_t> g_comm_idle;
static std::map<ncclComm_t, comm_key> g_comm_key;

static ncclResult_t comm_acquire(ncclComm_t *comm, int world, const void *id128, int rank)
{
    const comm_key key{std::string((const char *)id128, 128), world, rank};
    {
        std::lock_guard<std::mutex> lk(g_comm_mu);
        auto it = g_comm_idle.find(key);
        if (it != g_comm_idle.end()) {
            *comm = it->second;
            g_comm_idle.erase(it);
            return ncclSuccess;
        }
    }
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof id);
    const ncclResult_t r = ncclCommInitRank(comm, world, id, rank);
    if (r == ncclSuccess) {
        std::lock_guard<std::mutex> lk(g_comm_mu);
        g_comm_key[*comm] = key;
    }
    return r;
}

// idle communicators kept at most (a caller that makes a fresh unique id per
// solve and never calls vlgba_comm_release would otherwise keep one per rank
// per solve for the life of the process): past the cap one idle communicator
// of another id is destroyed, with a warning the first time
#ifndef BA_COMM_IDLE_CAP
#define BA_COMM_IDLE_CAP 64
#endif

static void comm_release(ncclComm_t comm)
{
    ncclComm_t evict = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_comm_mu);
        auto it = g_comm_key.find(comm);
        if (it == g_comm_key.end()) {
            evict = comm;   // its id was released while this context held it
        } else {
            const comm_key key = it->second;
            g_comm_idle.emplace(key, comm);
            if (g_comm_idle.size() > BA_COMM_IDLE_CAP) {
                for (auto q = g_comm_idle.begin(); q != g_comm_idle.end(); ++q)
                    if (q->first < key || key < q->first) {
                        evict = q->second;
                        g_comm_key.erase(evict);
                        g_comm_idle.erase(q);
                        break;
                    }
                static bool warned = false;
                if (evict && !warned) {
                    warned = true;
                    std::fprintf(stderr, "[vlgba] more than %d idle RCCL communicators: "
                                         "destroying the oldest ids' (call vlgba_comm_release "
                                         "for ids that will not be used again)\n",
                                 BA_COMM_IDLE_CAP);
                }
            }
        }
    }
    if (evict) ncclCommDestroy(evict);
}

static void kt_retire(const ba_ktimer *kt);

static void ctx_free(vlgba_ctx *c)
{
    if (!c) return;
    if (c->d.stream) (void)hipStreamSynchronize(c->d.stream);
    if (c->d.side) (void)hipStreamSynchronize(c->d.side);
    for (void *p : c->allocs) ba_dfree(p);
    for (void *p : {(void *)c->pinv_S, (void *)c->pinv_ev, (void *)c->pinv_e, (void *)c->pinv_w,
                    (void *)c->pinv_info})
        if (p) ba_dfree(p);
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

template <typename T>
static int ctx_alloc(vlgba_ctx *c, T **p, size_t count)
{
    TRY(dalloc(p, count));
    c->allocs.push_back((void *)*p);
    return 0;
}

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
    TRY(download(c->hb_tmp.data(), buf, count, c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    if (c->host_allreduce(c->hb_tmp.data(), (long long)count, c->host_user) != 0)
        return VLGBA_E_COMM;
    TRY(upload(buf, c->hb_tmp.data(), count, c->d.stream));
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
        TRY(ctx_alloc(c, &dev, total));
        ba_aux &x = c->aux;
        const size_t need = (total + sizeof(double) - 1) / sizeof(double);
        if (x.pin_cap < need) {
            if (x.pin) (void)hipHostFree(x.pin);
            size_t cap = 1 << 16;
            while (cap < need) cap <<= 1;
            x.pin = nullptr;
            x.pin_cap = 0;
            if (hipHostMalloc((void **)&x.pin, sizeof(double) * cap, hipHostMallocDefault) ==
                hipSuccess)
                x.pin_cap = cap;
        }
        char *stage = x.pin_cap >= need ? (char *)x.pin : nullptr;
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

    // local point-major arrays
    std::vector<int> lptr(d.n + 1), lcam(h.cam.begin() + o0, h.cam.begin() + o1);
    for (int i = 0; i <= d.n; i++) lptr[i] = pt_ptr_all[c->p0 + i] - (int)o0;
    // camera-major view of the local observations (obs ids ascending per camera)
    std::vector<int> cptr(p->m + 1, 0), cobs(d.N);
    for (int o = 0; o < d.N; o++) cptr[lcam[o] + 1]++;
    for (int j = 0; j < p->m; j++) cptr[j + 1] += cptr[j];
    {
        std::vector<int> pos(cptr.begin(), cptr.end() - 1);
        for (int o = 0; o < d.N; o++) cobs[pos[lcam[o]]++] = o;
    }
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
    plan_host(p->m, na, d.n, lptr, lcam, pt_ptr_all, h.cam, c->p0, c->p1, o0, lower_blocks,
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

    TRY(ctx_alloc(c, &d.obs_cam, d.N));
    TRY(ctx_alloc(c, &d.pt_ptr, d.n + 1));
    TRY(ctx_alloc(c, &d.cam_ptr, p->m + 1));
    TRY(ctx_alloc(c, &d.cam_obs, d.N));
    TRY(ctx_alloc(c, &d.obs_x, 2 * (size_t)d.N));
    TRY(ctx_alloc(c, &d.K4, 4 * (size_t)p->m));
    TRY(ctx_alloc(c, &d.a, (size_t)d.ld));
    TRY(ctx_alloc(c, &d.a_new, (size_t)d.ld));
    TRY(ctx_alloc(c, &d.b, 3 * (size_t)d.n));
    TRY(ctx_alloc(c, &d.b_new, 3 * (size_t)d.n));
    TRY(ctx_alloc(c, &d.rot, 45 * (size_t)p->m));
    TRY(ctx_alloc(c, &d.rot_new, 45 * (size_t)p->m));
    // W, eB, V*^-1 carry one zero row past the end: the MFMA Schur kernel points
    // the fragment loads of absent (point, camera) pairs at it
    TRY(ctx_alloc(c, &d.W, (size_t)3 * na * (d.N + 1)));
    VLGBA_CHECK(hipMemsetAsync(d.W + (size_t)3 * na * d.N, 0, sizeof(double) * 3 * na, s));
    if (!fast) {   // the fast path forms A, e, Y and t in LDS only
        TRY(ctx_alloc(c, &d.jrec, (size_t)d.js * d.N));
        TRY(ctx_alloc(c, &d.Y, (size_t)3 * na * d.N));
        TRY(ctx_alloc(c, &d.t, (size_t)na * d.N));
    } else {
        d.nch_reg = plan.nch_reg;
        d.nch = plan.nch_reg + plan.nseg;
        d.nl = (int)plan.long_pt.size();
        d.max_lcam = plan.max_lcam;
        d.long_o0_h = plan.long_o0.empty() ? 0 : plan.long_o0[0];
        d.p_long = p_long;
        // the plan's arrays: one device block, one copy (plan_batch)
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
            TRY(ctx_alloc(c, &d.ylong, (size_t)3 * na * plan.cam_lobs.size()));
            TRY(ctx_alloc(c, &d.vseg, 12 * (size_t)plan.nseg));
            TRY(ctx_alloc(c, &d.dpg_long, (size_t)d.nl));
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
        plan_obs_local_point(plan, lptr, lpt);
        plan_chunk_cameras(plan, lcam, ccam);
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
        TRY(ctx_alloc(c, &d.spart, (size_t)na * na * d.ngs));
        TRY(ctx_alloc(c, &d.epart, (size_t)na * d.nge));
        pb.add(&d.grp_ch, plan.grp_ch);
        pb.add(&d.grp_gs, plan.grp_gs);
        pb.add(&d.grp_ge, plan.grp_ge);
        pb.add(&d.cs_g, plan.cs_g);
        pb.add(&d.ce_g, plan.ce_g);
        pb.add(&d.blk_gptr, plan.blk_gptr);
        pb.add(&d.blk_gslots, plan.blk_gslots);
        pb.add(&d.cam_gptr, plan.cam_gptr);
        pb.add(&d.cam_gslots, plan.cam_gslots);
        TRY(ctx_alloc(c, &d.upart, (size_t)(na * (na + 1) / 2 + na) * d.nes));
        TRY(ctx_alloc(c, &d.chsse, 3 * (size_t)d.nch));   // lin SSE | new SSE | dpg
        pb.add(&d.ch_pt, plan.ch_pt);
        pb.add(&d.ch_eslot, plan.ch_eslot);
        pb.add(&d.eslot_optr, plan.eslot_optr);
        pb.add(&d.eslot_obs, plan.eslot_obs);
        pb.add(&d.cam_eptr, plan.cam_eptr);
        pb.add(&d.cam_eslots, plan.cam_eslots);
        TRY(pb.commit(c, s));   // (synchronous: the plan vectors are thread scratch)
        ST_MARK("plan_upload");
    }
    TRY(ctx_alloc(c, &d.U, (size_t)na * na * p->m + na * (size_t)p->m + 1));
    d.eA = d.U + (size_t)na * na * p->m;     // U | eA | old_sse contiguous: one all-reduce
    TRY(ctx_alloc(c, &d.V, 9 * (size_t)d.n));
    TRY(ctx_alloc(c, &d.eB, 3 * (size_t)(d.n + 1)));
    TRY(ctx_alloc(c, &d.Vinv, 9 * (size_t)(d.n + 1)));
    VLGBA_CHECK(hipMemsetAsync(d.eB + 3 * (size_t)d.n, 0, sizeof(double) * 3, s));
    VLGBA_CHECK(hipMemsetAsync(d.Vinv + 9 * (size_t)d.n, 0, sizeof(double) * 9, s));
    TRY(ctx_alloc(c, &d.db, 3 * (size_t)d.n));
    // fused update (fast path): the next linearisation's buffers (VLGBA_FUSED=0
    // keeps the separate update and linearisation launches: A/B)
    const char *fused_env = std::getenv("VLGBA_FUSED");   // read per context (tests)
    const bool fused_on = !(fused_env && fused_env[0] == '0');
    if (fast && d.nch > 0 && fused_on) {
        TRY(ctx_alloc(c, &d.W2, (size_t)3 * na * (d.N + 1)));
        VLGBA_CHECK(hipMemsetAsync(d.W2 + (size_t)3 * na * d.N, 0, sizeof(double) * 3 * na, s));
        TRY(ctx_alloc(c, &d.V2, 9 * (size_t)d.n));
        TRY(ctx_alloc(c, &d.eB2, 3 * (size_t)(d.n + 1)));
        VLGBA_CHECK(hipMemsetAsync(d.eB2 + 3 * (size_t)d.n, 0, sizeof(double) * 3, s));
        TRY(ctx_alloc(c, &d.upart2, (size_t)(na * (na + 1) / 2 + na) * d.nes));
        TRY(ctx_alloc(c, &d.chsse2, 3 * (size_t)d.nch));
        d.fused = 1;
    }
    TRY(ctx_alloc(c, &d.blk_jk, 2 * (size_t)d.nb));
    TRY(ctx_alloc(c, &d.blk_ptr, (size_t)d.nb + 1));
    TRY(ctx_alloc(c, &d.term, 2 * (size_t)d.T));
    TRY(upload(d.blk_jk, hb.jk.data(), hb.jk.size(), s));
    // the long tracks' pair counts per block (k_long_pairs) on the device while
    // the host builds the solve's structure (chol_plan_build); read back below
    int *lp_cnt = nullptr;
    if (fast && d.nl > 0) {
        TRY(ctx_alloc(c, &lp_cnt, (size_t)d.nb + 1));
        TRY(ctx_alloc(c, &d.lpair_ptr, (size_t)d.nb + 1));
        TRY(ba_launch_long_pairs(&d, 0, lp_cnt));
    }
    // blocks | rhs | old SSE contiguous: one all-reduce per pass (world > 1)
    TRY(ctx_alloc(c, &d.sblk, (size_t)na * na * d.nb + d.lds + 1));
    d.rhs = d.sblk + (size_t)na * na * d.nb;
    if (!stage_mode && d.dense_solve == 5) {
        // block-Jacobi PCG on sblk / rhs themselves: no dense S, no plan of the
        // direct solves (d.chol stays null), no direct assembly, no folded
        // camera update
        TRY(ctx_alloc(c, &d.da, (size_t)d.lds));
        ST_MARK("allocs");
        TRY(ba_pcg_setup(&d, hb.jk.data(), d.nb));
        ST_MARK("pcg_setup");
    } else if (!stage_mode) {
        TRY(ctx_alloc(c, &d.da, (size_t)d.lds));   // S, linv, ywork: ba_chol_setup
        ST_MARK("allocs");
        TRY(ba_chol_setup(&d, hb.jk.data(), d.nb));
        ST_MARK("chol_setup");
        // direct assembly (ba_dev::asm_direct): one rank without a collective
        // between the block sums and the solve, the fast path's block sums, no
        // long tracks (k_schur_long_acc adds to the sums after them);
        // VLGBA_ASM_DIRECT=0 keeps k_assemble_tiles (A/B)
        const chol_plan &P = d.chol->plan;
        const char *ad = std::getenv("VLGBA_ASM_DIRECT");
        d.asm_direct = P.asm_direct_ok && !(ad && ad[0] == '0') && fast && !d.ordered &&
                       c->world == 1 && !c->comm && d.nl == 0 && P.cr_nlev > 0 && P.cr32 &&
                       P.nd_np == 0;
        // camera update inside the one-launch CR (ba_dev::camupd_fold): x = da
        // in camera order, every tile a whole number of cameras, the Euclidean
        // models' rotation table, the fast path's final sums (k_sum_parts3);
        // VLGBA_CAMUPD_FOLD=0 keeps k_camera_update (A/B, tests)
        const char *cf = std::getenv("VLGBA_CAMUPD_FOLD");
        d.camupd_fold = !(cf && cf[0] == '0') && fast && !d.ordered && d.nch > 0 &&
                        P.cr_nlev > 0 && P.cr32 && P.cr_fused && d.chol->crflag && P.nd_np == 0 &&
                        na != BA_PROJ_NA && na <= 10 && P.tb32 % na == 0 &&
                        d.ld == (long long)na * p->m;
    } else {
        TRY(ctx_alloc(c, &d.da, (size_t)d.lds));
    }
    TRY(ctx_alloc(c, &d.part, 3 * (size_t)BA_PART_MAX));
    TRY(ctx_alloc(c, &d.scal, 8));
    TRY(upload(d.obs_cam, lcam.data(), d.N, s));
    TRY(upload(d.pt_ptr, lptr.data(), d.n + 1, s));
    TRY(upload(d.cam_ptr, cptr.data(), p->m + 1, s));
    TRY(upload(d.cam_obs, cobs.data(), d.N, s));
    TRY(upload(d.obs_x, h.x.data() + 2 * o0, 2 * (size_t)d.N, s));
    if (p->K) TRY(upload(d.K4, p->K, 4 * (size_t)p->m, s));
    else VLGBA_CHECK(hipMemsetAsync(d.K4, 0, sizeof(double) * 4 * p->m, s));
    TRY(upload(d.blk_ptr, hb.ptr.data(), hb.ptr.size(), s));
    TRY(upload(d.term, hb.term.data(), hb.term.size(), s));
    ST_MARK("uploads");
    if (fast && d.nl > 0) {   // the long tracks' per-block pair lists (k_long_pairs)
        std::vector<int> h((size_t)d.nb + 1, 0);
        TRY(download(h.data(), lp_cnt, (size_t)d.nb, s));
        VLGBA_CHECK(hipStreamSynchronize(s));
        long long tot = 0;
        for (int b = 0; b < d.nb; b++) {
            const int v = h[b];
            h[b] = (int)tot;
            tot += v;
        }
        h[d.nb] = (int)tot;
        if (tot > 0x7fffffffLL) return VLGBA_E_ARG;
        TRY(ctx_alloc(c, &d.lpair, (size_t)tot + 1));
        TRY(upload(d.lpair_ptr, h.data(), (size_t)d.nb + 1, s));
        TRY(ba_launch_long_pairs(&d, 1, nullptr));
        // the blocks with pairs for k_schur_long_acc, most pairs first
        // (VLGBA_LONG_ACC=0: k_schur_reduce streams them itself)
        const char *la = std::getenv("VLGBA_LONG_ACC");
        if (!(la && la[0] == '0')) {
            std::vector<int> lb;
            for (int b = 0; b < d.nb; b++)
                if (h[b + 1] > h[b]) lb.push_back(b);
            std::stable_sort(lb.begin(), lb.end(), [&](int x, int y) {
                return h[x + 1] - h[x] > h[y + 1] - h[y];
            });
            d.nlb = (int)lb.size();
            if (d.nlb > 0) {
                TRY(ctx_alloc(c, &d.lblk, lb.size()));
                TRY(upload(d.lblk, lb.data(), lb.size(), s));
            }
        }
        ST_MARK("long_pairs");
    }
    VLGBA_CHECK(hipMemsetAsync(d.scal, 0, 8 * sizeof(double), s));
    TRY(ctx_alloc(c, &d.pub_cnt, 1));
    VLGBA_CHECK(hipMemsetAsync(d.pub_cnt, 0, sizeof(unsigned), s));
    VLGBA_CHECK(hipStreamSynchronize(s));   // host vectors go out of scope
    return 0;
}

static int ctx_create(const vlgba_problem *p, const vlgba_options *o, vlgba_ctx **out,
                      bool lower_blocks, bool all_diag, bool stage_mode,
                      std::vector<int> *pt_ptr_out = nullptr, host_obs *h_out = nullptr)
{
    *out = nullptr;
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
    vlgba_ctx *c = new (std::nothrow) vlgba_ctx();
    if (!c) return VLGBA_E_NOMEM;
    std::memset(&c->d, 0, sizeof(c->d));
    vlgba_options defaults;
    std::memset(&defaults, 0, sizeof defaults);
    if (!o) o = &defaults;
    int rc = 0;
    setup_trace trace;
    g_st = &trace;
    struct st_reset { ~st_reset() { g_st = nullptr; } } st_reset_;
    do {
        if (hipSetDevice(o->device) != hipSuccess) { rc = VLGBA_E_ARG; break; }
        if (aux_acquire(o->device, c->aux)) {
            rc = -1;
            break;
        }
        c->has_aux = true;
        c->d.stream = c->aux.stream;
        c->d.side = c->aux.side;
        c->d.ev_fork = c->aux.ev_fork;
        c->d.ev_join = c->aux.ev_join;
        c->d.hres = c->aux.hres_host;
        c->d.hres_dev = c->aux.hres_dev;
        ST_MARK("aux");
        host_obs h;
        rc = sort_obs(p, h);
        if (rc) break;
        ST_MARK("sort");
        std::vector<int> pt_ptr_all(p->n + 1, 0);
        for (size_t q = 0; q < h.pt.size(); q++) pt_ptr_all[h.pt[q] + 1]++;
        for (int i = 0; i < p->n; i++) pt_ptr_all[i + 1] += pt_ptr_all[i];
        c->world = o->world_size > 1 ? o->world_size : 1;
        c->rank = c->world > 1 ? o->rank : 0;
        // contiguous point ranges with balanced observation counts
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
                if (comm_acquire(&c->comm, c->world, o->comm_id, c->rank) != ncclSuccess) {
                    rc = VLGBA_E_COMM;
                    break;
                }
            } else if (o->allreduce) {
                c->host_allreduce = o->allreduce;
                c->host_user = o->allreduce_user;
            } else {
                rc = VLGBA_E_COMM;
                break;
            }
        } else {
            c->p0 = 0;
            c->p1 = p->n;
            if (o->comm_id) {   // a one-rank RCCL communicator: every collective
                                // of the pass runs through RCCL (identity sums)
                if (comm_acquire(&c->comm, 1, o->comm_id, 0) != ncclSuccess) {
                    rc = VLGBA_E_COMM;
                    break;
                }
            }
        }
        // fast path: this rank's points by track kind (short tracks for the MFMA
        // Schur chunks first, per-term tracks, long tracks last); the ranges
        // of the other ranks are left as they are (the block set, the only
        // global structure a rank builds, is order independent: build_blocks)
        if (o->ordered == 0 && !stage_mode)
            order_points_by_kind(o->schur_kernel == 1 ? 0 : BA_MF_CMAX(p->num_a), h, pt_ptr_all,
                                 c->p0, c->p1, c->pperm, c->operm);
        ST_MARK("order");
        c->n_global = p->n;
        c->N_global = p->num_obs;
        c->num_vis = p->num_vis > 0 ? p->num_vis : (double)p->num_obs;
        c->flags.fix_structure = o->fix_structure;
        c->flags.fix_motion = o->fix_motion;
        if (o->semantics != 0 && o->semantics != 1) { rc = VLGBA_E_ARG; break; }
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
        if (o->dense_solve == 5 && (o->ordered != 0 || stage_mode)) { rc = VLGBA_E_ARG; break; }
        if (o->ordered == 2) {   // parity mode: + sequential solve and LM scalars
            if (c->world > 1) { rc = VLGBA_E_ARG; break; }
            c->d.parity = 1;
            c->d.dense_solve = 3;
        } else if (o->ordered < 0 || o->ordered > 2 || o->dense_solve < 0 ||
                   o->dense_solve > 5) {
            rc = VLGBA_E_ARG;
            break;
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
        rc = ctx_setup(c, p, h, pt_ptr_all, lower_blocks, all_diag, stage_mode);
        if (rc) break;
        // ... so a problem the planner hands to the ordered kernels is refused
        if (p->num_a == BA_RAD_NA && c->d.ordered) { rc = VLGBA_E_ARG; break; }
        if (c->d.pcg && c->d.ordered) { rc = VLGBA_E_ARG; break; }   // (the PCG likewise)
        ST_MARK("setup_end");
        if (c->d.parity) {   // new projections for the sequential new-SSE sum
            rc = ctx_alloc(c, &c->d.xh_out, 2 * (size_t)c->d.N + 2);
            if (rc) break;
        }
        if (c->flags.has_pivot) {
            rc = ctx_alloc(c, &c->d.pivot, (size_t)p->m);
            if (rc) break;
            rc = upload(c->d.pivot, o->pivot, (size_t)p->m, c->d.stream);
            if (rc) break;
        }
        if (std::getenv("VLGBA_KTIME_ALL")) {   // every context times its passes
            rc = vlgba_set_timing(c, 1);
            if (rc) break;
        }
        if (pt_ptr_out) *pt_ptr_out = pt_ptr_all;
        if (h_out) *h_out = std::move(h);
    } while (0);
    if (rc) {
        ctx_free(c);
        return rc;
    }
    *out = c;
    return 0;
}

// ---------------------------------------------------------------------------
// one LM pass
// ---------------------------------------------------------------------------
static inline void mark(vlgba_ctx *c, int q)
{
    if (c->timing) (void)hipEventRecord(c->ev[q], c->d.stream);
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
static int stage1(vlgba_ctx *c, int relinearize, camred_route route, stage1_left *left)
{
    ba_dev &d = c->d;
    const bool full = !c->lin_valid || (relinearize && !d.fused);
    if (full) TRY(ba_launch_linearize(&d, c->flags));
    mark(c, 1);
    if (!full && !relinearize && !c->camred_due) return 0;
    if (route == CAMRED_FOLD) {
        left->fold = true;
        left->fold_args = ba_camred_args(&d, c->flags);
    } else if (route == CAMRED_SIDE) {
        // (no collective in between at world size 1)
        VLGBA_CHECK(hipEventRecord(d.ev_fork, d.stream));
        VLGBA_CHECK(hipStreamWaitEvent(d.side, d.ev_fork, 0));
        TRY(ba_launch_camera_reduce(&d, c->flags, d.side));
        VLGBA_CHECK(hipEventRecord(d.ev_join, d.side));
        left->side_camred = true;
    } else {
        TRY(ba_launch_camera_reduce(&d, c->flags, d.stream));
    }
    // parity mode: the old SSE again, summed in the reference's flat order
    if (d.parity) TRY(ba_launch_parity_old_sse(&d));
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
static int schur_phase(vlgba_ctx *c, double lam, const stage1_left &left = {})
{
    ba_dev &d = c->d;
    mark(c, 2);
    if (d.ordered) {
        TRY(ba_launch_damp_point(&d, lam));
        mark(c, 3);
        TRY(ba_launch_schur(&d, lam));
    } else {
        mark(c, 3);
        TRY(ba_launch_schur_fast(&d, lam, left.fold ? &left.fold_args : nullptr,
                                 left.side_camred));
    }
    if (c->world > 1 || c->comm) {
        // [S blocks | e_ | old SSE] of this rank's points -> the global system
        double *sse = d.rhs + d.lds;
        VLGBA_CHECK(hipMemcpyAsync(sse, d.eA + d.ld, sizeof(double), hipMemcpyDeviceToDevice,
                                   d.stream));
        TRY(allreduce(c, d.sblk, (size_t)d.na * d.na * d.nb + d.lds + 1));
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
    if (c->world > 1 || c->comm) TRY(allreduce(c, d.scal + 1, 5));
    if (spin) {
        // spin on the host-mapped sequence number written last (by the update's
        // final sums, or k_publish); lower latency than a copy +
        // hipStreamSynchronize.  A stalled stream falls back to the
        // synchronisation, which reports the error
        if (!published) TRY(ba_launch_publish(&d));
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
    TRY(download(hs, d.scal, 6, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

// The end the recovery paths share: the update with the da they formed (never
// the one-launch CR's, so k_camera_update runs; nothing publishes), the parity
// sums, the scalars
static int recovery_update(vlgba_ctx *c, double lam, double hs[6])
{
    ba_dev &d = c->d;
    TRY(ba_launch_update(&d, lam, c->flags, false, false, nullptr));
    if (d.parity) TRY(ba_launch_parity_new_sums(&d, lam));
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
    TRY(ba_launch_assemble(&d));
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
    TRY(schur_phase(c, lam));
    // (a solve without spins never sets it; a PCG context solves again the same way)
    bool cam_updated = false;
    TRY(reduced_solve(c, &cam_updated, 1, false));
    TRY(recovery_update(c, lam, hs));
    c->spin_retries++;
    if (!d.chol) return 0;
    // one of the envelope runner's own hand-offs gave up (most likely its side
    // stream sharing a hardware queue with the library stream, so the column
    // launches queue behind it): this context's column launches alone from now on
    TRY(std::min(0, ba_env_runner_timed_out(&d)));
    return 0;
}

// rocSOLVER's symmetric eigensolver, loaded on first use (the library is
// ~0.9 GB; a pass that never meets a non-positive pivot never loads it)
namespace {
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
rs_api *rs_load()
{
    static rs_api api;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = dlopen("librocsolver.so.0", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librocsolver.so.0", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        api.create = (decltype(api.create))dlsym(h, "rocblas_create_handle");
        api.set_stream = (decltype(api.set_stream))dlsym(h, "rocblas_set_stream");
        api.syevd = (decltype(api.syevd))dlsym(h, "rocsolver_dsyevd");
        api.potrf = (decltype(api.potrf))dlsym(h, "rocsolver_dpotrf");
        api.potrs = (decltype(api.potrs))dlsym(h, "rocsolver_dpotrs");
        api.potri = (decltype(api.potri))dlsym(h, "rocsolver_dpotri");
        api.ok = api.create && api.set_stream && api.syevd;
    });
    return api.ok ? &api : nullptr;
}
std::mutex g_rs_mu;
std::map<int, rocblas_handle> g_rs_handle;   // per device
}   // namespace

// rocSOLVER, the dense scratch of the fallbacks and this device's handle
static int rs_prepare(vlgba_ctx *c, rs_api **rs_out, rocblas_handle *hdl_out)
{
    ba_dev &d = c->d;
    rs_api *rs = rs_load();
    if (!rs) return VLGBA_E_ARG;
    const long long ld = d.ld;
    if (ld > 0x7fffffffLL) return VLGBA_E_ARG;
    if (!c->pinv_S) {
        TRY(dalloc(&c->pinv_S, (size_t)(ld * ld)));
        TRY(dalloc(&c->pinv_ev, (size_t)ld));
        TRY(dalloc(&c->pinv_e, (size_t)ld));
        TRY(dalloc(&c->pinv_w, (size_t)ld));
        TRY(dalloc(&c->pinv_info, 1));
    }
    rocblas_handle hdl = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        auto it = g_rs_handle.find(d.device);
        if (it == g_rs_handle.end()) {
            if (rs->create(&hdl) != rocblas_status_success) return VLGBA_E_ARG;
            g_rs_handle[d.device] = hdl;
        } else {
            hdl = it->second;
        }
    }
    *rs_out = rs;
    *hdl_out = hdl;
    return 0;
}

// dpotrf / dpotri (fn) on the lower triangle of the dense scratch, in place,
// and its info word on the host.  The caller holds g_rs_mu and has set the
// handle's stream.
static int rs_factor_info(vlgba_ctx *c, rocblas_handle hdl, decltype(rs_api::potrf) fn, int *info)
{
    const rocblas_int ld = (rocblas_int)c->d.ld;
    if (fn(hdl, rocblas_fill_lower, ld, c->pinv_S, ld, c->pinv_info) != rocblas_status_success)
        return VLGBA_E_ARG;
    VLGBA_CHECK(hipMemcpyAsync(info, c->pinv_info, sizeof *info, hipMemcpyDeviceToHost,
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
    TRY(rs_prepare(c, &rs, &hdl));
    if (!rs->potrf || !rs->potrs) return 1;
    const long long ld = d.ld;
    TRY(schur_phase(c, lam));
    TRY(ba_launch_assemble_plain(&d, c->pinv_S, ld, 1));
    TRY(ba_fix_diag_plain(&d, c->pinv_S, ld));   // exactly-zero rows: unit diagonal, rhs 0
    VLGBA_CHECK(hipMemcpyAsync(c->pinv_e, d.rhs, sizeof(double) * ld, hipMemcpyDeviceToDevice,
                               d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    int info = 0;
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        if (rs->set_stream(hdl, d.stream) != rocblas_status_success) return VLGBA_E_ARG;
        TRY(rs_factor_info(c, hdl, rs->potrf, &info));
        if (info != 0) return 1;
        if (rs->potrs(hdl, rocblas_fill_lower, (rocblas_int)ld, 1, c->pinv_S, (rocblas_int)ld,
                      c->pinv_e, (rocblas_int)ld) != rocblas_status_success)
            return VLGBA_E_ARG;
    }
    VLGBA_CHECK(hipMemcpyAsync(d.da, c->pinv_e, sizeof(double) * ld, hipMemcpyDeviceToDevice,
                               d.stream));
    TRY(recovery_update(c, lam, hs));
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
    TRY(rs_prepare(c, &rs, &hdl));
    const long long ld = d.ld;
    TRY(schur_phase(c, lam));
    TRY(ba_launch_assemble_plain(&d, c->pinv_S, ld, 1));
    // the library stream is non-blocking: make S complete before rocSOLVER
    // (parts of dsyevd are ordered against the legacy stream, not ours)
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        if (rs->set_stream(hdl, d.stream) != rocblas_status_success ||
            rs->syevd(hdl, rocblas_evect_original, rocblas_fill_lower, (rocblas_int)ld,
                      c->pinv_S, (rocblas_int)ld, c->pinv_ev, c->pinv_e,
                      c->pinv_info) != rocblas_status_success)
            return VLGBA_E_ARG;
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
    }
    {
        int info = 0;
        VLGBA_CHECK(hipMemcpy(&info, c->pinv_info, sizeof info, hipMemcpyDeviceToHost));
        if (info != 0) return VLGBA_E_ARG;   // the eigensolver did not converge
    }
    TRY(ba_pinv_apply(&d, c->pinv_S, c->pinv_ev, ld, d.rhs, c->pinv_w, d.da));
    TRY(recovery_update(c, lam, hs));
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
    TRY(stage1(c, relinearize, route, &left));
    TRY(schur_phase(c, lam, left));
    mark(c, 4);
    bool cam_updated = false;   // the solve formed a_new / rot_new (one-launch CR)
    TRY(reduced_solve(c, &cam_updated, 0, true));
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
    TRY(ba_launch_update(&d, lam, c->flags, cam_updated, spin && !c->comm, &published));
    if (d.parity) TRY(ba_launch_parity_new_sums(&d, lam));
    mark(c, 7);
    // scalars: [0] old_sse [1] new_sse [2] dpg cameras [3] dpg points
    // [4] non-positive pivot [5] hand-off spin timeout (summed over ranks)
    double hs[6];
    TRY(collect_scalars(c, spin, published, hs));
    info->pinv = 0;
    info->spin_retry = 0;
    info->nd_retry = 0;
    if (hs[5] != 0.0) {   // the solve did not finish: again, without spins
        TRY(resolve_nospin(c, lam, hs));
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
        TRY(pinv_fallback(c, lam, hs));
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

// every handle entry point runs on the context's device, whatever the calling
// thread's current device is (allocations and launches follow hipGetDevice)
static int ctx_enter(vlgba_ctx *c)
{
    return hipSetDevice(c->aux.device) == hipSuccess ? 0 : VLGBA_E_ARG;
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

// the caller forgets a unique id: destroy the idle communicators made from it
// (contexts still holding one keep it until vlgba_destroy, which then
// destroys it as an unkeyed communicator).  Returns the number destroyed.
int vlgba_comm_release(const void *id128)
{
    if (!id128) return VLGBA_E_ARG;
    const std::string id((const char *)id128, 128);
    std::vector<ncclComm_t> drop;
    {
        std::lock_guard<std::mutex> lk(g_comm_mu);
        for (auto q = g_comm_idle.begin(); q != g_comm_idle.end();) {
            if (q->first.id == id) {
                drop.push_back(q->second);
                g_comm_key.erase(q->second);
                q = g_comm_idle.erase(q);
            } else {
                ++q;
            }
        }
        for (auto q = g_comm_key.begin(); q != g_comm_key.end();)   // in use: unkeyed,
            q = q->second.id == id ? g_comm_key.erase(q) : std::next(q);   // destroyed on release
    }
    for (ncclComm_t x : drop) ncclCommDestroy(x);
    return (int)drop.size();
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

// per-point device array (k doubles per local point, internal order) -> host,
// in the input point order (synchronous when a permutation applies)
static int download_points(vlgba_ctx *c, double *dst, const double *src, int k)
{
    const size_t cnt = (size_t)k * c->d.n;
    if (c->pperm.empty()) return download(dst, src, cnt, c->d.stream);
    std::vector<double> tmp(cnt);
    TRY(download(tmp.data(), src, cnt, c->d.stream));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    for (int i = 0; i < c->d.n; i++)
        std::memcpy(dst + (size_t)k * c->pperm[i], tmp.data() + (size_t)k * i, sizeof(double) * k);
    return 0;
}

int vlgba_set_params(vlgba_ctx *c, const double *a, const double *b)
{
    if (!c || !a || !b) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    static const bool pageable = std::getenv("VLGBA_SETP_PAGEABLE") != nullptr;   // A/B
    const size_t na = (size_t)c->d.ld, nb = 3 * (size_t)c->d.n;
    ba_aux &x = c->aux;
    if (!pageable && x.pin_cap < na + nb) {   // pinned staging: the copies start at once
        if (x.pin) (void)hipHostFree(x.pin);
        size_t cap = 1 << 16;
        while (cap < na + nb) cap <<= 1;
        x.pin = nullptr;
        x.pin_cap = 0;
        if (hipHostMalloc((void **)&x.pin, sizeof(double) * cap, hipHostMallocDefault) ==
            hipSuccess)
            x.pin_cap = cap;
    }
    double *ha = (!pageable && x.pin) ? x.pin : nullptr, *hb = ha ? ha + na : nullptr;
    if (ha) std::memcpy(ha, a, sizeof(double) * na);
    TRY(upload(c->d.a, ha ? ha : a, na, c->d.stream));
    if (!c->pperm.empty()) {   // input point order -> internal order
        double *dst = hb;
        if (!dst) {
            c->hb_tmp.resize(nb);
            dst = c->hb_tmp.data();
        }
        for (int i = 0; i < c->d.n; i++)
            for (int r = 0; r < 3; r++)
                dst[3 * (size_t)i + r] = b[3 * ((size_t)c->p0 + c->pperm[i]) + r];
        TRY(upload(c->d.b, dst, nb, c->d.stream));
    } else if (hb) {
        std::memcpy(hb, b + 3 * (size_t)c->p0, sizeof(double) * nb);
        TRY(upload(c->d.b, hb, nb, c->d.stream));
    } else {
        TRY(upload(c->d.b, b + 3 * (size_t)c->p0, nb, c->d.stream));
    }
    TRY(ba_launch_rotations(&c->d, c->d.a, c->d.rot));
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
    TRY(ctx_enter(c));
    if (a) TRY(download(a, c->d.a, (size_t)c->d.ld, c->d.stream));
    if (b) {
        if (c->world > 1) {
            // every rank returns the full b: all-reduce of a zero-padded copy
            double *full = nullptr;
            TRY(dalloc(&full, 3 * (size_t)c->n_global));
            VLGBA_CHECK(hipMemsetAsync(full, 0, sizeof(double) * 3 * c->n_global, c->d.stream));
            if (c->pperm.empty()) {
                VLGBA_CHECK(hipMemcpyAsync(full + 3 * (size_t)c->p0, c->d.b,
                                           sizeof(double) * 3 * c->d.n, hipMemcpyDeviceToDevice,
                                           c->d.stream));
            } else {   // internal -> input order inside this rank's range
                c->hb_tmp.resize(3 * (size_t)c->d.n);
                TRY(download_points(c, c->hb_tmp.data(), c->d.b, 3));
                VLGBA_CHECK(hipMemcpyAsync(full + 3 * (size_t)c->p0, c->hb_tmp.data(),
                                           sizeof(double) * 3 * c->d.n, hipMemcpyHostToDevice,
                                           c->d.stream));
                VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
            }
            int rc = allreduce(c, full, 3 * (size_t)c->n_global);
            if (!rc) rc = download(b, full, 3 * (size_t)c->n_global, c->d.stream);
            (void)hipStreamSynchronize(c->d.stream);
            ba_dfree(full);
            if (rc) return rc;
        } else {
            TRY(download_points(c, b, c->d.b, 3));
        }
    }
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

int vlgba_get_linearization(vlgba_ctx *c, double *U, double *eA, double *V, double *eB,
                            double *W)
{
    if (!c) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    ba_dev &d = c->d;
    // the linearisation the context holds for the current parameters (a
    // rejected step's, or the one the fused update made at an accepted step's
    // new point), else a new one
    TRY(stage1(c, 0, CAMRED_PLAIN, nullptr));
    // U / eA stay per-rank partials on the device (schur_owner); the caller
    // gets their sum over ranks
    const size_t nue = (size_t)d.na * d.na * d.m + d.ld + 1;
    double *ue = d.U;
    if (c->world > 1) {
        TRY(dalloc(&ue, nue));
        VLGBA_CHECK(hipMemcpyAsync(ue, d.U, sizeof(double) * nue, hipMemcpyDeviceToDevice,
                                   d.stream));
        const int rc = allreduce(c, ue, nue);
        if (rc) {
            ba_dfree(ue);
            return rc;
        }
    }
    int rc = 0;
    if (U) rc = download(U, ue, (size_t)d.na * d.na * d.m, d.stream);
    if (!rc && eA) rc = download(eA, ue + (size_t)d.na * d.na * d.m, (size_t)d.ld, d.stream);
    if (ue != d.U) {
        (void)hipStreamSynchronize(d.stream);
        ba_dfree(ue);
    }
    TRY(rc);
    if (V) TRY(download_points(c, V, d.V, 9));
    if (eB) TRY(download_points(c, eB, d.eB, 3));
    if (W) {
        if (c->operm.empty()) {
            TRY(download(W, d.W, (size_t)3 * d.na * d.N, d.stream));
        } else {   // internal observation order -> input order
            const size_t ws = (size_t)3 * d.na;
            std::vector<double> tmp(ws * d.N);
            TRY(download(tmp.data(), d.W, ws * d.N, d.stream));
            VLGBA_CHECK(hipStreamSynchronize(d.stream));
            for (int o = 0; o < d.N; o++)
                std::memcpy(W + ws * c->operm[o], tmp.data() + ws * o, sizeof(double) * ws);
        }
    }
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

int vlgba_get_reduced_system(vlgba_ctx *c, int *blk_jk, double *blocks, double *e_)
{
    if (!c) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    ba_dev &d = c->d;
    TRY(stage1(c, 0, CAMRED_PLAIN, nullptr));
    TRY(schur_phase(c, c->lambda));
    if (blk_jk) TRY(download(blk_jk, d.blk_jk, 2 * (size_t)d.nb, d.stream));
    if (blocks) TRY(download(blocks, d.sblk, (size_t)d.na * d.na * d.nb, d.stream));
    if (e_) TRY(download(e_, d.rhs, (size_t)d.ld, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    return 0;
}

// vlgba_covariance's per-context setup: the points binned by track length
// (ba_cov.hip) and the device buffers of its results
static int cov_setup(vlgba_ctx *c)
{
    ba_dev &d = c->d;
    if (c->cov_pts) return 0;
    std::vector<int> ptr((size_t)d.n + 1);
    TRY(download(ptr.data(), d.pt_ptr, (size_t)d.n + 1, d.stream));
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
    TRY(ctx_alloc(c, &c->cov_list, std::max<size_t>(1, list.size())));
    TRY(upload(c->cov_list, list.data(), list.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));   // list goes out of scope
    // VLGBA_COV_PACKED=0: the dense method's k_point_cov reads the dense inverse
    // (A/B); the packed copy is still filled, after the point kernel, for
    // vlgba_get_covariance_blocks
    const char *pk = std::getenv("VLGBA_COV_PACKED");
    c->cov_src_packed = !(pk && pk[0] == '0');
    {
        // the co-visible blocks (j >= k) by camera row j, columns ascending
        std::vector<int> jk(2 * (size_t)d.nb);
        TRY(download(jk.data(), d.blk_jk, jk.size(), d.stream));
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        std::vector<int> &ord = c->cov_ord;
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
        TRY(ctx_alloc(c, &c->cov_rowptr, rowptr.size()));
        TRY(ctx_alloc(c, &c->cov_col, std::max<size_t>(1, col.size())));
        TRY(ctx_alloc(c, &c->cov_bj, std::max<size_t>(1, bj.size())));
        TRY(upload(c->cov_rowptr, rowptr.data(), rowptr.size(), d.stream));
        TRY(upload(c->cov_col, col.data(), col.size(), d.stream));
        TRY(upload(c->cov_bj, bj.data(), bj.size(), d.stream));
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        // one block more than nb: the bisection of an empty row ends there
        TRY(ctx_alloc(c, &c->cov_packed, ((size_t)d.nb + 1) * d.na * d.na));
        VLGBA_CHECK(hipMemsetAsync(c->cov_packed, 0,
                                   sizeof(double) * ((size_t)d.nb + 1) * d.na * d.na, d.stream));
    }
    TRY(ctx_alloc(c, &c->cov_fixed, (size_t)std::max(1LL, d.ld)));
    TRY(ctx_alloc(c, &c->cov_diag, std::max<size_t>(1, (size_t)d.na * d.na * d.m)));
    c->cov_n8 = (int)bin[0].size();
    c->cov_n64 = (int)bin[1].size();
    c->cov_nwg = (int)bin[2].size();
    c->cov_tmax = tmax;
    c->cov_seen = seen;
    TRY(ctx_alloc(c, &c->cov_pts, std::max<size_t>(1, 9 * (size_t)d.n)));
    return 0;
}

// ... and of the selected method: the tile sources of its descent and its tiles
static int cov_setup_selected(vlgba_ctx *c)
{
    ba_dev &d = c->d;
    if (c->cov_sig) return 0;
    const int nt32 = d.chol->plan.nt32;   // (the selected method: a solving context)
    std::vector<int> src(2 * (size_t)nt32);
    TRY(ba_cr32_selinv_sources(&d, src.data()));
    TRY(ctx_alloc(c, &c->cov_selsrc, src.size()));
    TRY(upload(c->cov_selsrc, src.data(), src.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));   // src goes out of scope
    const size_t cnt = (size_t)3 * 32 * 32 * nt32;
    double *sig = nullptr;
    TRY(ctx_alloc(c, &sig, cnt));
    VLGBA_CHECK(hipMemsetAsync(sig, 0, sizeof(double) * cnt, d.stream));
    c->cov_sig = sig;
    return 0;
}

static int cov_run(vlgba_ctx *c, int scale, double *cov_a, double *cov_a_full, double *cov_b,
                   double *info)
{
    ba_dev &d = c->d;
    const bool sel = c->cov_method == VLGBA_COV_SELECTED;
    rs_api *rs = nullptr;
    rocblas_handle hdl = nullptr;
    if (!sel) {   // (the selected method needs neither rocSOLVER nor the dense scratch)
        TRY(rs_prepare(c, &rs, &hdl));
        if (!rs->potrf || !rs->potri) return VLGBA_E_ARG;
    }
    TRY(cov_setup(c));
    if (sel) TRY(cov_setup_selected(c));
    c->cov_have = 0;
    const long long ld = d.ld;
    TRY(stage1(c, 0, CAMRED_PLAIN, nullptr));
    hipEvent_t ev[3] = {};
    for (auto &e : ev) VLGBA_CHECK(hipEventCreate(&e));
    // the selected method: S0 in the CR's tiles as a pass assembles it (unit
    // diagonal on the exactly-zero rows), the fixed rows from the blocks, the
    // per-level factor launches, the descent, and the co-visible blocks out of
    // its tiles; no back substitution, da and the dense scratch untouched
    auto run_selected = [&]() -> int {
        VLGBA_CHECK(hipEventRecord(ev[0], d.stream));
        TRY(schur_phase(c, 0.0));
        TRY(ba_launch_assemble(&d));
        TRY(ba_cov_mark_fixed_blocks(&d, c->cov_fixed));
        TRY(ba_cr32_factor(&d));
        TRY(ba_cr32_selinv(&d, c->cov_selsrc, c->cov_sig));
        TRY(ba_cov_extract(&d, c->cov_sig, c->cov_fixed, c->cov_bj, c->cov_col, d.nb,
                           c->cov_diag, c->cov_packed));
        VLGBA_CHECK(hipEventRecord(ev[1], d.stream));
        const ba_cov_src src{nullptr, ld, c->cov_rowptr, c->cov_col, c->cov_packed};
        TRY(ba_launch_point_cov(&d, c->cov_list, c->cov_n8, c->cov_n64, c->cov_nwg, c->cov_tmax,
                                &src, c->cov_pts));
        VLGBA_CHECK(hipEventRecord(ev[2], d.stream));
        double pivot = 0.0;   // the CR's status word: a non-positive pivot
        TRY(download(&pivot, d.scal + 4, 1, d.stream));
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        return pivot != 0.0 ? VLGBA_E_SINGULAR : 0;
    };
    auto run = [&]() -> int {
        VLGBA_CHECK(hipEventRecord(ev[0], d.stream));
        // S0: the undamped Schur phase (it also leaves V+ = vlg_pinv3(V) in d.Vinv),
        // dense lower triangle, unit diagonal on the exactly-zero rows
        TRY(schur_phase(c, 0.0));
        TRY(ba_launch_assemble_plain(&d, c->pinv_S, ld, 1));
        TRY(ba_cov_mark_fixed(&d, c->pinv_S, ld, c->cov_fixed));
        TRY(ba_fix_diag_plain(&d, c->pinv_S, ld));
        // the library stream is non-blocking: S0 complete before rocSOLVER
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        {
            std::lock_guard<std::mutex> lk(g_rs_mu);
            int pinfo = 0;
            if (rs->set_stream(hdl, d.stream) != rocblas_status_success) return VLGBA_E_ARG;
            for (auto fn : {rs->potrf, rs->potri}) {
                TRY(rs_factor_info(c, hdl, fn, &pinfo));
                if (pinfo != 0) return VLGBA_E_SINGULAR;
            }
        }
        TRY(ba_cov_finish(&d, c->pinv_S, ld, c->cov_fixed, c->cov_diag));
        if (c->cov_src_packed)
            TRY(ba_cov_pack(&d, c->pinv_S, ld, c->cov_bj, c->cov_col, d.nb, c->cov_packed));
        VLGBA_CHECK(hipEventRecord(ev[1], d.stream));
        const ba_cov_src src{c->pinv_S, ld, c->cov_rowptr, c->cov_col,
                             c->cov_src_packed ? c->cov_packed : nullptr};
        TRY(ba_launch_point_cov(&d, c->cov_list, c->cov_n8, c->cov_n64, c->cov_nwg, c->cov_tmax,
                                &src, c->cov_pts));
        VLGBA_CHECK(hipEventRecord(ev[2], d.stream));
        if (!c->cov_src_packed)   // (for vlgba_get_covariance_blocks only)
            TRY(ba_cov_pack(&d, c->pinv_S, ld, c->cov_bj, c->cov_col, d.nb, c->cov_packed));
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        return 0;
    };
    int rc = sel ? run_selected() : run();
    float ms_a = 0.f, ms_b = 0.f;
    if (!rc) {
        (void)hipEventElapsedTime(&ms_a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms_b, ev[1], ev[2]);
    } else {
        (void)hipStreamSynchronize(d.stream);
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    TRY(rc);
    // SSE / dof: the linearisation's SSE (the old SSE of a pass from here)
    double sse = 0.0;
    std::vector<unsigned char> fixed((size_t)ld);
    TRY(download(&sse, d.eA + d.ld, 1, d.stream));
    TRY(download(fixed.data(), c->cov_fixed, (size_t)ld, d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    long long nfixed = 0;
    for (unsigned char f : fixed) nfixed += f;
    const double dof = 2.0 * (double)d.N -
                       ((double)(ld - nfixed) + (c->flags.fix_structure ? 0.0 : 3.0 * c->cov_seen));
    const double sigma2 = dof > 0 ? sse / dof : 0.0;
    if (info) {
        const double scratch = sel ? 8.0 * 3.0 * 32.0 * 32.0 * (double)d.chol->plan.nt32
                                   : 8.0 * (double)ld * (double)ld;
        const double v[8] = {sse, dof, sigma2, (double)nfixed, ms_a, ms_b, scratch, 0.0};
        std::memcpy(info, v, sizeof v);
    }
    if (scale && !(dof > 0)) return VLGBA_E_ARG;
    const size_t na2m = (size_t)d.na * d.na * d.m;
    if (cov_a) TRY(download(cov_a, c->cov_diag, na2m, d.stream));
    if (cov_a_full) TRY(download(cov_a_full, c->pinv_S, (size_t)(ld * ld), d.stream));
    if (cov_b) TRY(download_points(c, cov_b, c->cov_pts, 9));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    c->cov_have = 1;
    c->cov_scale = scale ? sigma2 : 1.0;
    if (scale) {
        for (size_t q = 0; cov_a && q < na2m; q++) cov_a[q] *= sigma2;
        for (size_t q = 0; cov_a_full && q < (size_t)(ld * ld); q++) cov_a_full[q] *= sigma2;
        for (size_t q = 0; cov_b && q < 9 * (size_t)d.n; q++) cov_b[q] *= sigma2;
    }
    return 0;
}

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
    if (cov_a_full && c->cov_method == VLGBA_COV_SELECTED) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
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

// the selected method runs on the camera-aligned cyclic reduction's factors
static bool cov_selected_ok(const vlgba_ctx *c)
{
    const ba_chol *ch = c->d.chol;   // (null in a stage-mode context: no factors)
    return ch && ch->plan.cr_nlev > 0 && ch->plan.cr32 && c->world == 1 && !c->comm &&
           !c->host_allreduce && !c->d.ordered;
}

int vlgba_set_covariance_method(vlgba_ctx *c, int kind)
{
    if (!c || (kind != VLGBA_COV_DENSE && kind != VLGBA_COV_SELECTED)) return VLGBA_E_ARG;
    if (kind == VLGBA_COV_SELECTED && !cov_selected_ok(c)) return VLGBA_E_ARG;
    c->cov_method = kind;
    return 0;
}

int vlgba_get_covariance_method(vlgba_ctx *c, int *kind)
{
    if (!c || !kind) return VLGBA_E_ARG;
    *kind = c->cov_method;
    return 0;
}

int vlgba_get_covariance_blocks(vlgba_ctx *c, int *blk_jk, double *blocks)
{
    if (!c || !c->cov_have || !c->cov_packed) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    ba_dev &d = c->d;
    const size_t nn = (size_t)d.na * d.na;
    if (blk_jk) TRY(download(blk_jk, d.blk_jk, 2 * (size_t)d.nb, d.stream));
    std::vector<double> pk(blocks ? nn * d.nb : 0);
    if (blocks) TRY(download(pk.data(), c->cov_packed, pk.size(), d.stream));
    VLGBA_CHECK(hipStreamSynchronize(d.stream));
    // packed block p (by camera row, columns ascending) is block cov_ord[p]
    for (int p = 0; blocks && p < d.nb; p++) {
        double *o = blocks + nn * (size_t)c->cov_ord[p];
        for (size_t q = 0; q < nn; q++) o[q] = pk[nn * p + q] * c->cov_scale;
    }
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
    TRY(ctx_enter(c));
    c->d.jac = kind;
    // the table of the current a in the new mode's layout; a camera update the
    // last solve folded in built the other one
    TRY(ba_launch_rotations(&c->d, c->d.a, c->d.rot));
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
    TRY(ctx_enter(c));
    ba_dev &d = c->d;
    const size_t N = (size_t)d.N;
    if (N == 0 || (!e && !w && !rho)) return 0;
    double *buf = nullptr;   // e [N][2] | w [N] | rho [N], internal observation order
    TRY(dalloc(&buf, 4 * N));
    auto run = [&]() -> int {
        // the rotation table of d.a is current (set_params / an accepted step)
        TRY(ba_launch_obs_residuals(&d, e ? buf : nullptr, w ? buf + 2 * N : nullptr,
                                    rho ? buf + 3 * N : nullptr));
        double *dst[3] = {e, w, rho};
        const size_t off[3] = {0, 2 * N, 3 * N}, wd[3] = {2, 1, 1};
        std::vector<double> tmp;
        for (int q = 0; q < 3; q++) {
            if (!dst[q]) continue;
            if (c->operm.empty()) {
                TRY(download(dst[q], buf + off[q], wd[q] * N, d.stream));
                continue;
            }
            tmp.resize(wd[q] * N);   // internal observation order -> input order
            TRY(download(tmp.data(), buf + off[q], wd[q] * N, d.stream));
            VLGBA_CHECK(hipStreamSynchronize(d.stream));
            for (size_t o = 0; o < N; o++)
                std::memcpy(dst[q] + wd[q] * c->operm[o], tmp.data() + wd[q] * o,
                            sizeof(double) * wd[q]);
        }
        VLGBA_CHECK(hipStreamSynchronize(d.stream));
        return 0;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(d.stream);
    ba_dfree(buf);
    return rc;
}

int vlgba_get_step(vlgba_ctx *c, double *da, double *db)
{
    if (!c) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    if (da) TRY(download(da, c->d.da, (size_t)c->d.ld, c->d.stream));
    if (db) TRY(download_points(c, db, c->d.db, 3));
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
    TRY(ctx_enter(c));
    if (on && !c->ev[0])
        for (auto &e : c->ev) VLGBA_CHECK(hipEventCreate(&e));
    if (on && !c->d.kt) {
        c->d.kt = new (std::nothrow) ba_ktimer();
        if (!c->d.kt) return VLGBA_E_NOMEM;
    }
    c->timing = on;
    if (c->d.kt) c->d.kt->on = on;
    return 0;
}

// kernel times of the contexts destroyed with timing on (VLGBA_KTIME_ALL=1:
// every context times its passes -- the growing replay's device-busy split)
static std::mutex g_kt_mu;
static double g_kt_ms[KT_N], g_kt_flops[KT_N];
static long long g_kt_calls[KT_N];

static void kt_retire(const ba_ktimer *kt)
{
    std::lock_guard<std::mutex> lk(g_kt_mu);
    for (int k = 0; k < KT_N; k++) {
        g_kt_ms[k] += kt->ms[k];
        g_kt_calls[k] += kt->calls[k];
        g_kt_flops[k] += kt->flops[k];
    }
}

int vlgba_kernel_ms(vlgba_ctx *c, double *ms, long long *calls, int reset)
{
    if (!c) {   // process-wide: the destroyed contexts' timers
        std::lock_guard<std::mutex> lk(g_kt_mu);
        for (int k = 0; k < KT_N; k++) {
            if (ms) ms[k] = g_kt_ms[k];
            if (calls) calls[k] = g_kt_calls[k];
            if (reset) {
                g_kt_ms[k] = 0.0;
                g_kt_calls[k] = 0;
                g_kt_flops[k] = 0.0;
            }
        }
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
        std::lock_guard<std::mutex> lk(g_kt_mu);
        for (int k = 0; k < KT_N; k++) flops[k] = g_kt_flops[k];
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
    TRY(ctx_enter(c));
    VLGBA_CHECK(hipStreamSynchronize(c->d.stream));
    return 0;
}

int vlgba_step(vlgba_ctx *c, int relinearize, int update_lm, vlgba_step_info *info)
{
    if (!c) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    vlgba_step_info tmp;
    if (!info) info = &tmp;
    TRY(lm_pass(c, relinearize, info));
    if (update_lm) lm_apply(c, info);
    return 0;
}

int vlgba_run_passes(vlgba_ctx *c, int npass, vlgba_step_info *info)
{
    if (!c || npass < 0) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
    vlgba_step_info tmp;
    if (!info) info = &tmp;
    std::memset(info, 0, sizeof *info);
    for (int q = 0; q < npass; q++) TRY(lm_pass(c, 1, info));
    return 0;
}

// bundle_euclid.m:111-249
int vlgba_run(vlgba_ctx *c, double *error_out, int error_cap, vlgba_stats *stats)
{
    if (!c || (error_out && error_cap < 0)) return VLGBA_E_ARG;
    TRY(ctx_enter(c));
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
        TRY(lm_pass(c, 0, &info));
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
    TRY(vlgba_create(prob, opt, &c));
    int rc = vlgba_set_params(c, a, b);
    if (!rc) rc = vlgba_run(c, error_out, error_cap, stats);
    if (!rc) rc = vlgba_get_params(c, a, b);
    vlgba_destroy(c);
    return rc;
}

// ---------------------------------------------------------------------------
// stage entries (MEX layouts)
// ---------------------------------------------------------------------------
static void obs_from_vis(int m, int n, const double *vis, std::vector<int> &pt,
                         std::vector<int> &cam)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++)
            if (vis[i + (size_t)n * j] != 0.0) {
                pt.push_back(i);
                cam.push_back(j);
            }
}

static int mex1_impl(int model, int m, int n, int num_a, const double *K, const double *a,
                     const double *b, const double *X, const double *vis, double *X_hat,
                     double *A, double *B, double *e, double *U, double *V, double *W,
                     double *eA, double *eB)
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
    vlgba_problem pr = {m, n, num_a, N, pt.data(), cam.data(), ox.data(), K, 0.0, model};
    vlgba_ctx *c = nullptr;
    TRY(ctx_create(&pr, nullptr, &c, true, true, true));
    ba_dev &d = c->d;
    int rc = 0;
    std::vector<double> jr((size_t)d.js * N), hW((size_t)3 * num_a * N), xh(2 * N), hB(6 * N);
    do {
        if ((rc = ctx_alloc(c, &d.xh_out, 2 * (size_t)N))) break;
        if ((rc = ctx_alloc(c, &d.B_out, 6 * (size_t)N))) break;
        if ((rc = upload(d.a, a, (size_t)d.ld, d.stream))) break;
        if ((rc = upload(d.b, b, 3 * (size_t)n, d.stream))) break;
        ba_flags f = {0, 0, 0};
        if ((rc = ba_launch_rotations(&d, d.a, d.rot))) break;
        if ((rc = ba_launch_linearize(&d, f))) break;
        if ((rc = ba_launch_camera_reduce(&d, f, d.stream))) break;
        if ((rc = download(jr.data(), d.jrec, jr.size(), d.stream))) break;
        if ((rc = download(hW.data(), d.W, hW.size(), d.stream))) break;
        if ((rc = download(xh.data(), d.xh_out, xh.size(), d.stream))) break;
        if ((rc = download(hB.data(), d.B_out, hB.size(), d.stream))) break;
        if ((rc = download(U, d.U, (size_t)num_a * num_a * m, d.stream))) break;
        if ((rc = download(eA, d.eA, (size_t)num_a * m, d.stream))) break;
        if ((rc = download(V, d.V, 9 * (size_t)n, d.stream))) break;
        if ((rc = download(eB, d.eB, 3 * (size_t)n, d.stream))) break;
        if (hipStreamSynchronize(d.stream) != hipSuccess) { rc = -1; break; }
    } while (0);
    ctx_free(c);
    if (rc) return rc;
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

static int mex2_impl(int model, int m, int n, int num_a, const double *Y, const double *W,
                     const double *U, const double *eA, const double *eB, double *S,
                     double *e_)
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
    std::vector<double> K(4 * (size_t)m, 1.0);
    vlgba_problem pr = {m, n, num_a, N, pt.data(), cam.data(), ox.data(), K.data(), 0.0, model};
    vlgba_ctx *c = nullptr;
    TRY(ctx_create(&pr, nullptr, &c, false, true, true));
    ba_dev &d = c->d;
    const long long ld = d.ld;
    int rc = 0;
    double *Sd = nullptr;
    do {
        if ((rc = ctx_alloc(c, &Sd, (size_t)(ld * ld)))) break;
        if ((rc = upload(d.Y, hY.data(), hY.size(), d.stream))) break;
        if ((rc = upload(d.W, hW.data(), hW.size(), d.stream))) break;
        if ((rc = upload(d.U, U, (size_t)num_a * num_a * m, d.stream))) break;
        if ((rc = upload(d.eA, eA, (size_t)num_a * m, d.stream))) break;
        if ((rc = upload(d.eB, eB, 3 * (size_t)n, d.stream))) break;
        if ((rc = ba_launch_yeb(&d))) break;
        // U is given already damped (bundle_euclid.m:192 passes U_): lambda = 0
        if ((rc = ba_launch_schur(&d, 0.0))) break;
        if ((rc = ba_launch_assemble_plain(&d, Sd, ld, 0))) break;
        if ((rc = download(S, Sd, (size_t)(ld * ld), d.stream))) break;
        if ((rc = download(e_, d.rhs, (size_t)ld, d.stream))) break;
        if (hipStreamSynchronize(d.stream) != hipSuccess) { rc = -1; break; }
    } while (0);
    ctx_free(c);
    return rc;
}

static int mex3_impl(int model, int m, int n, int num_a, const double *W, const double *da,
                     const double *eB, const double *Vinv, const double *K, const double *a,
                     const double *b, const double *X, const double *vis, double *db,
                     double *a_new, double *b_new, double *X_hat)
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
    vlgba_problem pr = {m, n, num_a, N, pt.data(), cam.data(), ox.data(), K, 0.0, model};
    vlgba_ctx *c = nullptr;
    TRY(ctx_create(&pr, nullptr, &c, true, true, true));
    ba_dev &d = c->d;
    int rc = 0;
    do {
        if ((rc = ctx_alloc(c, &d.xh_out, 2 * (size_t)N))) break;
        if ((rc = ctx_alloc(c, &d.obs_vis, (size_t)N))) break;
        if ((rc = upload(d.obs_vis, ov.data(), ov.size(), d.stream))) break;
        if ((rc = upload(d.W, hW.data(), hW.size(), d.stream))) break;
        if ((rc = upload(d.da, da, (size_t)d.ld, d.stream))) break;
        if ((rc = upload(d.eB, eB, 3 * (size_t)n, d.stream))) break;
        if ((rc = upload(d.Vinv, Vinv, 9 * (size_t)n, d.stream))) break;
        if ((rc = upload(d.a, a, (size_t)d.ld, d.stream))) break;
        if ((rc = upload(d.b, b, 3 * (size_t)n, d.stream))) break;
        VLGBA_CHECK(hipMemsetAsync(d.eA, 0, sizeof(double) * d.ld, d.stream));
        if ((rc = ba_launch_update(&d, 0.0, ba_flags{}, false, false, nullptr))) break;
        if ((rc = download(db, d.db, 3 * (size_t)n, d.stream))) break;
        if ((rc = download(a_new, d.a_new, (size_t)d.ld, d.stream))) break;
        if ((rc = download(b_new, d.b_new, 3 * (size_t)n, d.stream))) break;
        if ((rc = download(xh.data(), d.xh_out, xh.size(), d.stream))) break;
        if (hipStreamSynchronize(d.stream) != hipSuccess) { rc = -1; break; }
    } while (0);
    ctx_free(c);
    if (rc) return rc;
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
    double *buf = nullptr;
    int *info = nullptr;
    const size_t n = (size_t)ld;
    TRY(dalloc(&buf, n * n + 4 * n));
    int rc = dalloc(&info, 1);
    rocblas_handle hdl = nullptr;
    do {
        if (rc) break;
        double *A = buf, *ev = buf + n * n, *e = ev + n, *w = e + n, *rhs = w + n;
        if (hipMemcpy(A, S, sizeof(double) * n * n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(rhs, e_, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) {
            rc = -1;
            break;
        }
        if (rs->create(&hdl) != rocblas_status_success ||
            rs->syevd(hdl, rocblas_evect_original, rocblas_fill_lower, ld, A, ld, ev, e, info) !=
                rocblas_status_success) {
            rc = VLGBA_E_ARG;
            break;
        }
        if ((rc = ba_pinv_apply(&d, A, ev, ld, rhs, w, e))) break;
        if (hipMemcpy(da, e, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    } while (0);
    (void)hipDeviceSynchronize();
    if (hdl) {
        auto destroy = (rocblas_status(*)(rocblas_handle))dlsym(RTLD_DEFAULT,
                                                                 "rocblas_destroy_handle");
        if (destroy) destroy(hdl);
    }
    ba_dfree(buf);
    if (info) ba_dfree(info);
    return rc;
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

}  // extern "C"
