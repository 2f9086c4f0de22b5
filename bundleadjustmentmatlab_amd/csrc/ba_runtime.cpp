// ba_runtime.cpp -- libvlgba's process-wide resources: the caching device
// allocator and the dynamic-LDS cache, the kernel timers and their totals, the
// pooled streams / events / pinned blocks of the contexts, the RCCL
// communicator pool, the rocSOLVER loader and its per-device handles.  Host
// code only; nothing here knows the LM.
#include "ba_ctx.h"

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>

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

// VLGBA_POISON=1 (debugging): every block handed out is filled with 0xff
// bytes (NaN doubles, -1 ints), so a kernel that reads memory it never wrote
// shows up as NaN instead of as a stale value of a previous context
void *poisoned(void *p, size_t b)
{
    static const bool on = std::getenv("VLGBA_POISON") != nullptr;
    if (on && p) {   // null-stream memset: not ordered with non-blocking streams
        (void)hipMemset(p, 0xff, b);
        (void)hipDeviceSynchronize();
    }
    return p;
}
}   // namespace

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

// ---------------------------------------------------------------------------
// kernel timers
// ---------------------------------------------------------------------------
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

// kernel times of the contexts destroyed with timing on (VLGBA_KTIME_ALL=1:
// every context times its passes -- the growing replay's device-busy split)
static std::mutex g_kt_mu;
static double g_kt_ms[KT_N], g_kt_flops[KT_N];
static long long g_kt_calls[KT_N];

void kt_retire(const ba_ktimer *kt)
{
    std::lock_guard<std::mutex> lk(g_kt_mu);
    for (int k = 0; k < KT_N; k++) {
        g_kt_ms[k] += kt->ms[k];
        g_kt_calls[k] += kt->calls[k];
        g_kt_flops[k] += kt->flops[k];
    }
}

void kt_totals(double *ms, long long *calls, double *flops, int reset)
{
    std::lock_guard<std::mutex> lk(g_kt_mu);
    for (int k = 0; k < KT_N; k++) {
        if (ms) ms[k] = g_kt_ms[k];
        if (calls) calls[k] = g_kt_calls[k];
        if (flops) flops[k] = g_kt_flops[k];
        if (reset) {
            g_kt_ms[k] = 0.0;
            g_kt_calls[k] = 0;
            g_kt_flops[k] = 0.0;
        }
    }
}

// ---------------------------------------------------------------------------
// Per-device pool of the context's streams, fork/join events and host-mapped
// result block: creating them (pinned host memory above all) costs ~0.4 ms,
// which the growing-BA replay would pay per solve.  A context takes one set
// for its lifetime and returns it idle (both streams synchronised).
// ---------------------------------------------------------------------------
static std::mutex g_aux_mu;
static std::vector<ba_aux> g_aux_pool;

int aux_acquire(int device, ba_aux &a)
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

void aux_release(const ba_aux &a)
{
    (void)hipStreamSynchronize(a.stream);
    (void)hipStreamSynchronize(a.side);
    std::lock_guard<std::mutex> lk(g_aux_mu);
    g_aux_pool.push_back(a);
}

double *aux_pin(ba_aux &a, size_t doubles)
{
    if (a.pin_cap < doubles) {
        if (a.pin) (void)hipHostFree(a.pin);
        size_t cap = 1 << 16;
        while (cap < doubles) cap <<= 1;
        a.pin = nullptr;
        a.pin_cap = 0;
        if (hipHostMalloc((void **)&a.pin, sizeof(double) * cap, hipHostMallocDefault) ==
            hipSuccess)
            a.pin_cap = cap;
    }
    return a.pin_cap >= doubles ? a.pin : nullptr;
}

// ---------------------------------------------------------------------------
// RCCL communicators outlive their context, keyed by (unique id, world size,
// rank): a caller that passes the same id again (dist.run_sharded keeps one
// id per device set for a whole growing replay) takes the idle communicator
// instead of paying ncclCommInitRank per solve.  One context per key at a
// time.  An idle communicator is destroyed only when its caller says the id
// is done (vlgba_comm_release): a unique id serves ONE bootstrap, so evicting
// the communicator of an id the caller may pass again would send that next
// context into an ncclCommInitRank that waits forever.
// ---------------------------------------------------------------------------
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

ncclResult_t comm_acquire(ncclComm_t *comm, int world, const void *id128, int rank)
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

void comm_release(ncclComm_t comm)
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

// the caller forgets a unique id: destroy the idle communicators made from it
// (contexts still holding one keep it until vlgba_destroy, which then
// destroys it as an unkeyed communicator).  Returns the number destroyed.
int comm_forget(const void *id128)
{
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

// ---------------------------------------------------------------------------
// rocSOLVER's symmetric eigensolver and Cholesky routines, loaded on first use
// (the library is ~0.9 GB; a pass that never meets a non-positive pivot never
// loads it)
// ---------------------------------------------------------------------------
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
static std::map<int, rocblas_handle> g_rs_handle;   // per device

// rocSOLVER and this device's handle
int rs_prepare(int device, rs_api **rs_out, rocblas_handle *hdl_out)
{
    rs_api *rs = rs_load();
    if (!rs) return VLGBA_E_ARG;
    rocblas_handle hdl = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        auto it = g_rs_handle.find(device);
        if (it == g_rs_handle.end()) {
            if (rs->create(&hdl) != rocblas_status_success) return VLGBA_E_ARG;
            g_rs_handle[device] = hdl;
        } else {
            hdl = it->second;
        }
    }
    *rs_out = rs;
    *hdl_out = hdl;
    return 0;
}
