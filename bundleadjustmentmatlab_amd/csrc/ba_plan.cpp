// ba_plan.cpp -- the context's host planner (ba_plan.h): observation sort,
// co-visible blocks, point order by track kind, and the chunk / group plan of
// the fast Schur path, built on the planner's own worker threads.  The plan
// is the same bit for bit on any thread count (tests/test_plan_threads.py).
// Host only: compiled without the HIP language or a ROCm include path.
#include "ba_plan.h"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

int sort_obs(const vlgba_problem *p, host_obs &h)
{
    const long long N = p->num_obs;
    // already point-major with cameras ascending within a point (the growing
    // replay's subsets, bundle_euclid's visibility order): a copy
    bool sorted = true;
    for (long long o = 0; o < N && sorted; o++) {
        const int i = p->obs_pt[o], j = p->obs_cam[o];
        if (i < 0 || i >= p->n || j < 0 || j >= p->m) return VLGBA_E_ARG;
        if (o > 0) {
            const int i0 = p->obs_pt[o - 1], j0 = p->obs_cam[o - 1];
            if (i < i0 || (i == i0 && j < j0)) sorted = false;
            else if (i == i0 && j == j0) return VLGBA_E_ORDER;
        }
    }
    if (sorted) {
        h.pt.assign(p->obs_pt, p->obs_pt + N);
        h.cam.assign(p->obs_cam, p->obs_cam + N);
        h.x.assign(p->obs_x, p->obs_x + 2 * N);
        return 0;
    }
    std::vector<long long> cnt(p->n + 1, 0);
    for (long long o = 0; o < N; o++) {
        const int i = p->obs_pt[o], j = p->obs_cam[o];
        if (i < 0 || i >= p->n || j < 0 || j >= p->m) return VLGBA_E_ARG;
        cnt[i + 1]++;
    }
    for (int i = 0; i < p->n; i++) cnt[i + 1] += cnt[i];
    std::vector<long long> pos(cnt.begin(), cnt.end() - 1);
    std::vector<long long> perm(N);
    for (long long o = 0; o < N; o++) perm[pos[p->obs_pt[o]]++] = o;
    h.pt.resize(N);
    h.cam.resize(N);
    h.x.resize(2 * N);
    for (int i = 0; i < p->n; i++) {
        std::sort(perm.begin() + cnt[i], perm.begin() + cnt[i + 1],
                  [&](long long u, long long v) { return p->obs_cam[u] < p->obs_cam[v]; });
        for (long long q = cnt[i]; q < cnt[i + 1]; q++) {
            const long long o = perm[q];
            if (q > cnt[i] && p->obs_cam[o] == h.cam[q - 1]) return VLGBA_E_ORDER;
            h.pt[q] = i;
            h.cam[q] = p->obs_cam[o];
            h.x[2 * q] = p->obs_x[2 * o];
            h.x[2 * q + 1] = p->obs_x[2 * o + 1];
        }
    }
    return 0;
}

void build_blocks(int m, const std::vector<int> &pt_ptr_all, const std::vector<int> &cam_all,
                  int p0, int p1, long long obs_base, bool lower, bool all_diag, bool need_terms,
                  host_blocks &hb)
{
    const int n = (int)pt_ptr_all.size() - 1;
    hb.m = m;
    hb.dense_tab = (long long)m * m <= (1LL << 26);
    if (hb.dense_tab && hb.tab.size() < (size_t)m * m)   // (else all -1 already: reset)
        hb.tab.assign((size_t)m * m, -1);
    else hb.rows.resize(m);
    auto find = [&](int j, int k) -> int { return hb.find(j, k); };
    // canonical block ids, (k, j) ascending: independent of the point order,
    // so ranks that order their own points differently (order_points_by_kind)
    // agree on the packed layout of the all-reduced blocks
    if (lower && hb.dense_tab) {
        // the lower block set as one bit row per column k (bit j: block (j, k),
        // j >= k), each point's cameras OR-ed in as a word mask over the span
        // of its track (cameras ascending within a point): O(track x span / 64)
        // per point instead of one table insert per camera pair, then the ids
        // handed out row by row = (k, j) ascending
        const int nw = (m + 63) / 64;
        std::vector<unsigned long long> rowb((size_t)m * nw, 0ull), mask(nw, 0ull);
        if (all_diag)
            for (int j = 0; j < m; j++) rowb[(size_t)j * nw + (j >> 6)] |= 1ull << (j & 63);
        for (int i = 0; i < n; i++) {
            const int a0 = pt_ptr_all[i], a1 = pt_ptr_all[i + 1];
            if (a1 <= a0) continue;
            const int w0 = cam_all[a0] >> 6, w1 = cam_all[a1 - 1] >> 6;
            for (int a = a0; a < a1; a++) mask[cam_all[a] >> 6] |= 1ull << (cam_all[a] & 63);
            for (int a = a0; a < a1; a++) {
                unsigned long long *row = &rowb[(size_t)cam_all[a] * nw];
                for (int w = w0; w <= w1; w++) row[w] |= mask[w];
            }
            for (int w = w0; w <= w1; w++) mask[w] = 0ull;
        }
        for (int k = 0; k < m; k++) {
            const unsigned long long *row = &rowb[(size_t)k * nw];
            for (int w = k >> 6; w < nw; w++) {
                unsigned long long bits = row[w];
                if (w == (k >> 6)) bits &= ~0ull << (k & 63);   // j >= k only
                while (bits) {
                    const int j = 64 * w + __builtin_ctzll(bits);
                    bits &= bits - 1;
                    hb.tab[(size_t)j * m + k] = (int)hb.jk.size() / 2;
                    hb.jk.push_back(j);
                    hb.jk.push_back(k);
                }
            }
        }
    } else {
        if (all_diag)
            for (int j = 0; j < m; j++) hb.insert(j, j);
        for (int i = 0; i < n; i++)
            for (int a = pt_ptr_all[i]; a < pt_ptr_all[i + 1]; a++)
                for (int b = pt_ptr_all[i]; b < pt_ptr_all[i + 1]; b++) {
                    const int j = cam_all[a], k = cam_all[b];
                    if (lower && j < k) continue;
                    hb.insert(j, k);
                }
        const int nb0 = (int)hb.jk.size() / 2;
        std::vector<int> ord(nb0);
        std::iota(ord.begin(), ord.end(), 0);
        std::sort(ord.begin(), ord.end(), [&](int u, int v) {
            const int ku = hb.jk[2 * u + 1], kv = hb.jk[2 * v + 1];
            return ku != kv ? ku < kv : hb.jk[2 * u] < hb.jk[2 * v];
        });
        std::vector<int> jk2(2 * (size_t)nb0);
        for (int q = 0; q < nb0; q++) {
            jk2[2 * q] = hb.jk[2 * ord[q]];
            jk2[2 * q + 1] = hb.jk[2 * ord[q] + 1];
        }
        hb.jk.swap(jk2);
        if (hb.dense_tab) {
            for (int q = 0; q < nb0; q++) hb.tab[(size_t)hb.jk[2 * q] * m + hb.jk[2 * q + 1]] = q;
        } else {
            for (auto &r : hb.rows) r.clear();
            for (int q = 0; q < nb0; q++) hb.rows[hb.jk[2 * q]].push_back({hb.jk[2 * q + 1], q});
        }
    }
    const int nb = (int)hb.jk.size() / 2;
    if (!need_terms) {
        hb.ptr.assign(nb + 1, 0);
        return;
    }
    std::vector<long long> cnt(nb + 1, 0);
    for (int i = p0; i < p1; i++)
        for (int a = pt_ptr_all[i]; a < pt_ptr_all[i + 1]; a++)
            for (int b = pt_ptr_all[i]; b < pt_ptr_all[i + 1]; b++) {
                const int j = cam_all[a], k = cam_all[b];
                if (lower && j < k) continue;
                cnt[find(j, k) + 1]++;
            }
    for (int q = 0; q < nb; q++) cnt[q + 1] += cnt[q];
    hb.ptr.resize(nb + 1);
    for (int q = 0; q <= nb; q++) hb.ptr[q] = (int)cnt[q];
    hb.term.resize(2 * (size_t)cnt[nb]);
    std::vector<long long> pos(cnt.begin(), cnt.end() - 1);
    for (int i = p0; i < p1; i++)   // points ascending => terms ascending per block
        for (int a = pt_ptr_all[i]; a < pt_ptr_all[i + 1]; a++)
            for (int b = pt_ptr_all[i]; b < pt_ptr_all[i + 1]; b++) {
                const int j = cam_all[a], k = cam_all[b];
                if (lower && j < k) continue;
                const long long s = pos[find(j, k)]++;
                hb.term[2 * s] = (int)(a - obs_base);
                hb.term[2 * s + 1] = (int)(b - obs_base);
            }
}

namespace {

static int plan_threads(long long work, long long min_work);
template <typename F>
static void parallel_ranges(int n, int nthr, F f, const std::vector<long long> *wpre);

// counting sort of ids by key: ptr[nkey+1], list of ids in ascending id order
// per key (large inputs: per-thread counts over contiguous id ranges, each
// thread's ids placed after those of the ranges before it: the same order)
static void bucket(const std::vector<int> &key, int nkey, std::vector<int> &ptr,
                   std::vector<int> &list)
{
    const int n = (int)key.size();
    const int T = std::min(plan_threads(n, 200000), std::max(1, (int)(4LL * n / (nkey + 1))));
    ptr.assign(nkey + 1, 0);
    list.resize(key.size());
    if (T <= 1) {
        for (int k : key) ptr[k + 1]++;
        for (int q = 0; q < nkey; q++) ptr[q + 1] += ptr[q];
        std::vector<int> pos(ptr.begin(), ptr.end() - 1);
        for (int s = 0; s < n; s++) list[pos[key[s]]++] = s;
        return;
    }
    std::vector<std::vector<int>> cnt(T);
    parallel_ranges(n, T, [&](int t, int s0, int s1) {
        cnt[t].assign(nkey, 0);
        for (int s = s0; s < s1; s++) cnt[t][key[s]]++;
    }, nullptr);
    for (int k = 0; k < nkey; k++) {   // cnt[t][k] <- start of thread t's ids of key k
        int at = ptr[k];
        for (int t = 0; t < T; t++) {
            const int c = cnt[t][k];
            cnt[t][k] = at;
            at += c;
        }
        ptr[k + 1] = at;
    }
    parallel_ranges(n, T, [&](int t, int s0, int s1) {
        std::vector<int> &pos = cnt[t];
        for (int s = s0; s < s1; s++) list[pos[key[s]]++] = s;
    }, nullptr);
}

// phase times of build_plan on stderr (tools/bench_plan.sh builds with it)
#ifdef BA_PLAN_TIMING
#define PLAN_T0 auto plan_t0_ = std::chrono::steady_clock::now()
#define PLAN_T(w)                                                                           \
    do {                                                                                    \
        const auto t_ = std::chrono::steady_clock::now();                                   \
        std::fprintf(stderr, "   %-14s %7.2f ms\n", w,                                     \
                     std::chrono::duration<double, std::milli>(t_ - plan_t0_).count());     \
        plan_t0_ = t_;                                                                      \
    } while (0)
#else
#define PLAN_T0
#define PLAN_T(w)
#endif

// Host threads of a context's plan: VLGBA_HOST_THREADS, else OMP_NUM_THREADS
// (the GPU box's CPU share), else the hardware's, at most 16; fewer when the
// work has fewer than min_work items per thread.
static int plan_threads(long long work, long long min_work)
{
    static const int cap = [] {
        int v = 0;
        if (const char *e = std::getenv("VLGBA_HOST_THREADS")) v = std::atoi(e);
        if (v <= 0)
            if (const char *e = std::getenv("OMP_NUM_THREADS")) v = std::atoi(e);
        if (v <= 0) v = (int)std::thread::hardware_concurrency();
        return std::max(1, std::min(v, 16));
    }();
    return (int)std::max(1LL, std::min<long long>(cap, work / std::max(1LL, min_work)));
}

// The host planner's worker threads: created once and kept (a context is
// created per growing-replay solve, and spawning 15 threads per plan phase
// cost more than some phases).  Two pools, one job each at a time: the
// replay builds two contexts side by side (its two prefetch workers); a
// caller that finds both busy (more concurrent creations, e.g. rank
// threads), or a forked child (the pools' threads stayed in the parent), runs
// its job on threads of its own instead.
class plan_pool {
  public:
    // f(t) for t in [0, nthr): t = 0 on the calling thread; false (nothing
    // run) if this pool is busy or unusable here
    bool try_run(int nthr, const std::function<void(int)> &f)
    {
        std::unique_lock<std::mutex> busy(job_mu_, std::defer_lock);
        if (getpid() != pid_ || nthr - 1 > kMax || !busy.try_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            while ((int)th_.size() < nthr - 1) {
                const int id = (int)th_.size() + 1;
                th_.emplace_back([this, id] { loop(id); });
            }
            job_ = &f;
            njob_ = nthr;
            pending_ = nthr - 1;
            gen_++;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
        return true;
    }

  private:
    static constexpr int kMax = 15;
    void loop(int id)
    {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)> *f = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (id < njob_) f = job_;
            }
            if (!f) continue;
            (*f)(id);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    const pid_t pid_ = getpid();
    std::mutex job_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int)> *job_ = nullptr;
    int njob_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
};

static void plan_run(int nthr, const std::function<void(int)> &f)
{
    static plan_pool *pools = new plan_pool[2];   // never destroyed: no join at exit
    for (int q = 0; q < 2; q++)
        if (pools[q].try_run(nthr, f)) return;
    std::vector<std::thread> th;   // threads of our own
    for (int t = 1; t < nthr; t++) th.emplace_back(f, t);
    f(0);
    for (auto &x : th) x.join();
}

// f(t, lo, hi) on nthr contiguous ranges of [0, n) (thread t takes range t;
// the calling thread takes range 0), of equal work when wpre (the prefix sums
// of per-item work, n + 1 entries) is given, else of equal length
template <typename F>
static void parallel_ranges(int n, int nthr, F f, const std::vector<long long> *wpre)
{
    if (nthr <= 1) {
        f(0, 0, n);
        return;
    }
    std::vector<int> cut(nthr + 1, n);
    cut[0] = 0;
    for (int t = 1; t < nthr; t++) {
        if (wpre) {
            const long long target = (*wpre)[n] * t / nthr;
            cut[t] = (int)(std::lower_bound(wpre->begin(), wpre->begin() + n + 1, target) -
                           wpre->begin());
        } else {
            cut[t] = (int)((long long)n * t / nthr);
        }
        cut[t] = std::max(cut[t], cut[t - 1]);
    }
    plan_run(nthr, [&](int t) { f(t, cut[t], cut[t + 1]); });
}

// MFMA chunks (points below p_split): at most BA_MF_PTS points and cmax
// cameras per chunk (the chunk's dense Y / W fit one K = 64 slab of
// 16 * BA_MF_RT(na) rows); their metadata records are the dense-layout ones
// described at build of P.blob below.
bool build_plan(int m, int na, const std::vector<int> &lptr, const std::vector<int> &lcam,
                const host_blocks &hb, host_plan &P, int cmax, int p_split, int p_long)
{
    const int n_all = (int)lptr.size() - 1;
    const int n = p_long;   // regular chunks cover points [0, p_long)
    const int nb = (int)hb.jk.size() / 2;
    if (cmax <= 0) p_split = 0;
    auto pt_terms = [&](int i) {
        const long long k = lptr[i + 1] - lptr[i];
        return k * (k + 1) / 2;
    };
    for (int i = 0; i < n; i++)
        if (lptr[i + 1] - lptr[i] > BA_CH_OBS || pt_terms(i) > BA_CH_TERMS ||
            (i < p_split && lptr[i + 1] - lptr[i] > cmax))
            return false;
    PLAN_T0;
    // chunk boundaries (sequential: the MFMA chunking follows the camera sets)
    std::vector<int> cbeg, cend;
    std::vector<char> cmf;
    {
        std::vector<int> cam_stamp(m, -1);   // chunk camera set (MFMA chunking)
        P.max_terms = 0;
        int p = 0;
        while (p < n) {
            const bool mf = p < p_split;                // chunk kind
            const int pend = mf ? p_split : n;
            const int pts_max = mf ? BA_MF_PTS : BA_CH_PTS;
            const int obase = lptr[p];
            int q = p;
            long long nterm = 0;
            int ncam = 0;
            bool uniform = true;   // every point so far sees exactly the first point's cameras
            auto same_cams = [&](int i1, int i2) {
                if (lptr[i1 + 1] - lptr[i1] != lptr[i2 + 1] - lptr[i2]) return false;
                for (int a = 0; a < lptr[i1 + 1] - lptr[i1]; a++)
                    if (lcam[lptr[i1] + a] != lcam[lptr[i2] + a]) return false;
                return true;
            };
            while (q < pend && q - p < pts_max && lptr[q + 1] - obase <= BA_CH_OBS &&
                   nterm + pt_terms(q) <= BA_CH_TERMS) {
                if (mf) {
                    // a run of points with one camera list (video-like tracks) keeps
                    // its chunks to itself: its MFMA sums stay in registers across
                    // chunks
                    const bool same = q == p || same_cams(p, q);
                    if (uniform && !same && q - p >= 4) break;
                    uniform = uniform && same;
                    int add = 0;
                    for (int a = lptr[q]; a < lptr[q + 1]; a++) add += cam_stamp[lcam[a]] != p;
                    if (ncam + add > cmax) break;
                    for (int a = lptr[q]; a < lptr[q + 1]; a++) cam_stamp[lcam[a]] = p;
                    ncam += add;
                }
                nterm += pt_terms(q++);
            }
            P.max_terms = std::max(P.max_terms, (int)nterm);
            P.n_terms += nterm;
            cbeg.push_back(p);
            cend.push_back(q);
            cmf.push_back(mf ? 1 : 0);
            p = q;
        }
    }
    PLAN_T("boundaries");
    // per chunk, in parallel over ranges of chunks (each thread's output is
    // contiguous in chunk order, so the ranges concatenate to the sequential
    // plan): pass 1 the chunk's slots (co-visible blocks, by first touch) and
    // e-slots (cameras) with their term / observation counts; pass 2 the
    // per-term lists (term chunks only: the MFMA records are dense) and the
    // per-camera observation lists, grouped by slot / e-slot in that order
    const int nchk = (int)cbeg.size();
    // (cache-line aligned: every push_back writes a vector header, and the
    // headers of neighbouring threads' outputs must not share a line)
    struct alignas(128) chunk_out {
        std::vector<int> blk, tcnt, cam, ecnt, ns, nes;
        std::vector<unsigned short> term, eobs;
        void clear()
        {
            for (std::vector<int> *v : {&blk, &tcnt, &cam, &ecnt, &ns, &nes}) v->clear();
            term.clear();
            eobs.clear();
        }
    };
    std::vector<long long> cwork(nchk + 1, 0);   // per chunk: its terms and observations
    for (int c = 0; c < nchk; c++) {
        long long w = lptr[cend[c]] - lptr[cbeg[c]];
        for (int i = cbeg[c]; i < cend[c]; i++) w += pt_terms(i);
        cwork[c + 1] = cwork[c] + w;
    }
    const int nthr = plan_threads(cwork[nchk], 20000);
    // the per-thread outputs live in the calling thread's scratch (capacity kept
    // from one context to the next: no page faults on the replay's plans)
    // (a reference: the pool threads' lambda must reach THIS thread's scratch,
    // not their own thread_local instance)
    static thread_local std::vector<chunk_out> co_tl;
    std::vector<chunk_out> &co = co_tl;
    if ((int)co.size() < nthr) co.resize(nthr);
    for (chunk_out &o : co) o.clear();
#ifdef BA_PLAN_TIMING
    std::vector<double> thr_ms(nthr, 0.0), thr_start(nthr, 0.0);
    PLAN_T("chunks prep");
    const auto tpr0 = std::chrono::steady_clock::now();
#endif
    parallel_ranges(nchk, nthr, [&](int t, int c0, int c1) {
#ifdef BA_PLAN_TIMING
        const auto tt0 = std::chrono::steady_clock::now();
        thr_start[t] = std::chrono::duration<double, std::milli>(tt0 - tpr0).count();
        struct tdone {
            std::chrono::steady_clock::time_point t0;
            double *out;
            ~tdone()
            {
                *out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                                 t0).count();
            }
        } tdone_{tt0, &thr_ms[t]};
#endif
        chunk_out &o = co[t];
        // per chunk: its cameras' local ids (e-slots, by first touch) and a
        // local nes x nes table of slot ids -- one global block lookup per
        // camera pair of the chunk instead of two per (obs, obs) term (the
        // m x m table does not stay in cache at ~1000 cameras); slots are
        // still numbered by first touch in (point, a, b) order
        std::vector<int> eslot_of(m, -1), tpos, epos, le, lslot;
        for (int c = c0; c < c1; c++) {
            const int p = cbeg[c], q = cend[c], obase = lptr[p], nob = lptr[q] - obase;
            const bool mf = cmf[c] != 0;
            const size_t s0 = o.blk.size(), e0 = o.cam.size();
            le.resize(nob);
            for (int a = obase; a < obase + nob; a++) {
                const int j = lcam[a];
                if (eslot_of[j] < 0) {
                    eslot_of[j] = (int)(o.cam.size() - e0);
                    o.cam.push_back(j);
                    o.ecnt.push_back(0);
                }
                o.ecnt[e0 + eslot_of[j]]++;
                le[a - obase] = eslot_of[j];
            }
            const int nce = (int)(o.cam.size() - e0);
            lslot.assign((size_t)nce * nce, -1);
            for (int i = p; i < q; i++)
                for (int a = lptr[i]; a < lptr[i + 1]; a++) {
                    const int j = lcam[a], ea = le[a - obase];
                    for (int b = lptr[i]; b < lptr[i + 1]; b++) {
                        const int k = lcam[b];
                        if (j < k) continue;
                        int &sl = lslot[(size_t)ea * nce + le[b - obase]];
                        if (sl < 0) {
                            sl = (int)(o.blk.size() - s0);
                            o.blk.push_back(hb.find(j, k));
                            o.tcnt.push_back(0);
                        }
                        o.tcnt[s0 + sl]++;
                    }
                }
            const int ns = (int)(o.blk.size() - s0), nes = (int)(o.cam.size() - e0);
            o.ns.push_back(ns);
            o.nes.push_back(nes);
            tpos.assign(ns + 1, 0);
            epos.assign(nes + 1, 0);
            for (int sl = 0; sl < ns; sl++) {
                if (mf) o.tcnt[s0 + sl] = 0;   // the MFMA records are dense: no term lists
                tpos[sl + 1] = tpos[sl] + o.tcnt[s0 + sl];
            }
            for (int e = 0; e < nes; e++) epos[e + 1] = epos[e] + o.ecnt[e0 + e];
            const size_t tb = o.term.size() / 2, ub = o.eobs.size();
            o.term.resize(2 * (tb + tpos[ns]));
            o.eobs.resize(ub + epos[nes]);
            for (int i = p; i < q; i++)
                for (int a = lptr[i]; a < lptr[i + 1]; a++) {
                    const int j = lcam[a], ea = le[a - obase];
                    o.eobs[ub + epos[ea]++] = (unsigned short)(a - obase);
                    if (mf) continue;
                    for (int b = lptr[i]; b < lptr[i + 1]; b++) {
                        if (j < lcam[b]) continue;
                        const size_t at = tb + tpos[lslot[(size_t)ea * nce + le[b - obase]]]++;
                        o.term[2 * at] = (unsigned short)(a - obase);
                        o.term[2 * at + 1] = (unsigned short)(b - obase);
                    }
                }
            for (size_t e = e0; e < o.cam.size(); e++) eslot_of[o.cam[e]] = -1;
        }
    }, &cwork);
#ifdef BA_PLAN_TIMING
    std::fprintf(stderr, "   (chunk threads:");
    for (int q = 0; q < nthr; q++) std::fprintf(stderr, " %.2f+%.2f", thr_start[q], thr_ms[q]);
    std::fprintf(stderr, " ms)\n");
#endif
    PLAN_T("chunks");
    // concatenate in chunk order: every thread's output block has a known
    // offset (sizes summed in thread order), so the blocks are copied -- and
    // their slot / e-slot prefix sums and chunk ranges formed -- in parallel
    // (element by element push_backs cost ~2 ms at cfg5x-900, sequentially)
    {
        const int NO = (int)co.size();
        std::vector<size_t> ob(NO + 1, 0), oc(NO + 1, 0), ot(NO + 1, 0), ou(NO + 1, 0),
            och(NO + 1, 0);
        for (int t = 0; t < NO; t++) {
            ob[t + 1] = ob[t] + co[t].blk.size();
            oc[t + 1] = oc[t] + co[t].cam.size();
            ot[t + 1] = ot[t] + co[t].term.size();
            ou[t + 1] = ou[t] + co[t].eobs.size();
            och[t + 1] = och[t] + co[t].ns.size();
        }
        P.slot_blk.resize(ob[NO]);
        P.slot_tptr.resize(ob[NO] + 1);
        P.cam_eslots.resize(oc[NO]);
        P.eslot_optr.resize(oc[NO] + 1);
        P.slot_term.resize(ot[NO]);
        P.eslot_obs.resize(ou[NO]);
        P.ch_pt.resize(och[NO] + 1);
        P.ch_slot.resize(och[NO] + 1);
        P.ch_eslot.resize(och[NO] + 1);
        P.slot_tptr[0] = P.eslot_optr[0] = 0;
        P.ch_pt[0] = P.ch_slot[0] = P.ch_eslot[0] = 0;
        std::vector<int> tmax(NO, 0);
        auto copy_block = [&](int t) {
            const chunk_out &o = co[t];
            std::copy(o.blk.begin(), o.blk.end(), P.slot_blk.begin() + ob[t]);
            int acc = (int)(ot[t] / 2);   // term pairs before this block
            for (size_t q = 0; q < o.tcnt.size(); q++) P.slot_tptr[ob[t] + 1 + q] = acc += o.tcnt[q];
            std::copy(o.cam.begin(), o.cam.end(), P.cam_eslots.begin() + oc[t]);
            acc = (int)ou[t];
            for (size_t q = 0; q < o.ecnt.size(); q++) P.eslot_optr[oc[t] + 1 + q] = acc += o.ecnt[q];
            std::copy(o.term.begin(), o.term.end(), P.slot_term.begin() + ot[t]);
            std::copy(o.eobs.begin(), o.eobs.end(), P.eslot_obs.begin() + ou[t]);
            int sa = (int)ob[t], ea = (int)oc[t];
            for (size_t u = 0; u < o.ns.size(); u++) {
                const size_t c = och[t] + u;
                tmax[t] = std::max(tmax[t], o.ns[u]);
                P.ch_pt[c + 1] = cend[c];
                P.ch_slot[c + 1] = sa += o.ns[u];
                P.ch_eslot[c + 1] = ea += o.nes[u];
            }
        };
        const int nct = std::min(NO, plan_threads((long long)(ob[NO] + ot[NO] + ou[NO]), 50000));
        plan_run(nct, [&](int w) {
            for (int t = w; t < NO; t += nct) copy_block(t);
        });
        P.max_slots = 0;
        for (int t = 0; t < NO; t++) P.max_slots = std::max(P.max_slots, tmax[t]);
        for (int c = 0; c < nchk; c++)
            if (cmf[c]) P.nch_mf++;
    }
    PLAN_T("concat");
    // long tracks: segment chunks (one point each, <= BA_CH_OBS observations;
    // every observation its own camera slot: a point sees a camera once)
    P.nch_reg = (int)P.ch_pt.size() - 1;
    P.long_o0.assign(1, lptr[p_long]);
    P.long_seg0.assign(1, 0);
    for (int i = p_long; i < n_all; i++) {
        const int l = (int)P.long_pt.size();
        P.long_pt.push_back(i);
        for (int o = lptr[i]; o < lptr[i + 1]; o += BA_CH_OBS) {
            const int o1 = std::min(o + BA_CH_OBS, lptr[i + 1]);
            for (int a = o; a < o1; a++) {
                P.eslot_obs.push_back((unsigned short)(a - o));
                P.eslot_optr.push_back((int)P.eslot_obs.size());
                P.cam_eslots.push_back(lcam[a]);
            }
            P.ch_eslot.push_back((int)P.eslot_optr.size() - 1);
            P.seg_pt.push_back(i);
            P.seg_long.push_back(l);
            P.nseg++;
        }
        P.long_o0.push_back(lptr[i + 1]);
        P.long_seg0.push_back(P.nseg);
    }
    // per camera: its e-slots in chunk order (cam_eslots currently = camera of
    // e-slot) -- a counting sort that keeps the id order (bucket: threads over
    // id ranges for large inputs).  (The per-block lists of the chunk slots are
    // not built: the block sums read the group slots, blk_gptr / blk_gslots.)
    std::vector<int> ecam;
    ecam.swap(P.cam_eslots);
    bucket(ecam, m, P.cam_eptr, P.cam_eslots);
    const int ns = (int)P.slot_blk.size(), nes = (int)P.eslot_optr.size() - 1;
    PLAN_T("blk lists");
    // Schur groups (greedy): at most gs_cap distinct blocks (LDS accumulators),
    // BA_GE_CAP cameras and gmax chunks (>= ~2048 groups keep the chip busy).
    // A chunk with more than gs_cap blocks forms a group of its own whose
    // partials go straight to HBM ("direct" group).
    const int nch = (int)P.ch_pt.size() - 1;
    std::vector<int> gslot_of(nb, -1), gcam_of(m, -1);
    P.cs_g.assign(ns, 0);
    P.ce_g.assign(nes, 0);
    P.grp_ch.assign(1, 0);
    P.grp_gs.assign(1, 0);
    P.grp_ge.assign(1, 0);
    // The MFMA segment's chunks are spread evenly over BA_MF_GROUPS groups
    // (fractional: group k ends near chunk (k + 1) nseg / G): one workgroup
    // per slot of k_schur_mfma's 3 x 256 CUs, no partly filled last round
    // (config 3: 1953 groups of 13 chunks -- 2.54 rounds -- took 179-183 us,
    // 1536 groups 167-169, 768 groups 155; 1024 / 2304 / 3072: 182-187,
    // profiles/r05i_*, r05j_*).  The term segment keeps BA_GROUPS' cap.
    // VLGBA_SCHUR_GROUPS overrides G (measurement).
    static const int Genv = [] {
        const char *e = std::getenv("VLGBA_SCHUR_GROUPS");
        const int v = e ? std::atoi(e) : 0;
        return v > 0 ? v : 0;
    }();
    int seg0 = 0, kseg = 0;
    for (int c = 0; c < nch;) {
        const bool mf = c < P.nch_mf;
        const int cend = mf ? P.nch_mf : nch, nseg = mf ? P.nch_mf : nch - P.nch_mf;
        if (c == 0 || c == P.nch_mf) seg0 = c, kseg = 0;
        // the MFMA kernel has no direct mode: one chunk's blocks must always fit
        const int gs_cap = mf ? std::max(BA_MF_GACC / (na * na), cmax * (cmax + 1) / 2)
                              : BA_GACC / (na * na);
        const int G = Genv ? Genv : (mf ? BA_MF_GROUPS : 0);
        const long long tend = G ? seg0 + ((long long)(kseg + 1) * nseg + G - 1) / G : 0;
        const int gmax = G ? (int)std::min<long long>(BA_GROUP_CH, std::max<long long>(1, tend - c))
                           : std::min(BA_GROUP_CH, std::max(1, (nseg + BA_GROUPS - 1) / BA_GROUPS));
        kseg++;
        const int ge_cap = mf ? std::max(BA_MF_GE_CAP, cmax) : BA_GE_CAP;
        if (gmax == 1) {
            // one chunk per group: its slots and e-slots are distinct blocks /
            // cameras already, so the group's lists are the chunk's (what the
            // general loop below builds, without its table lookups)
            const int s0 = P.ch_slot[c], s1 = P.ch_slot[c + 1];
            const int e0 = P.ch_eslot[c], e1 = P.ch_eslot[c + 1];
            P.gslot_blk.insert(P.gslot_blk.end(), P.slot_blk.begin() + s0,
                               P.slot_blk.begin() + s1);
            for (int q = s0; q < s1; q++) P.cs_g[q] = (unsigned short)(q - s0);
            P.gecam.insert(P.gecam.end(), ecam.begin() + e0, ecam.begin() + e1);
            for (int q = e0; q < e1; q++) P.ce_g[q] = (unsigned short)(q - e0);
            const int ngs_ = s1 - s0, nge_ = e1 - e0;
            if (mf) {
                P.mf_max_s = std::max(P.mf_max_s, ngs_);
                P.mf_max_e = std::max(P.mf_max_e, nge_);
                P.ngrp_mf++;
            } else if (ngs_ <= gs_cap) {
                P.grp_max_s = std::max(P.grp_max_s, ngs_);
                P.grp_max_e = std::max(P.grp_max_e, nge_);
            }
            P.grp_ch.push_back(c + 1);
            P.grp_gs.push_back((int)P.gslot_blk.size());
            P.grp_ge.push_back((int)P.gecam.size());
            c++;
            continue;
        }
        std::vector<int> gs, ge;
        int d = c;
        for (; d < cend && d - c < gmax; d++) {
            int new_s = 0, new_e = 0;
            for (int s = P.ch_slot[d]; s < P.ch_slot[d + 1]; s++) new_s += gslot_of[P.slot_blk[s]] < 0;
            for (int e = P.ch_eslot[d]; e < P.ch_eslot[d + 1]; e++) new_e += gcam_of[ecam[e]] < 0;
            if (d > c && ((int)gs.size() + new_s > gs_cap || (int)ge.size() + new_e > ge_cap))
                break;
            for (int s = P.ch_slot[d]; s < P.ch_slot[d + 1]; s++) {
                const int b = P.slot_blk[s];
                if (gslot_of[b] < 0) {
                    gslot_of[b] = (int)gs.size();
                    gs.push_back(b);
                }
                P.cs_g[s] = (unsigned short)gslot_of[b];
            }
            for (int e = P.ch_eslot[d]; e < P.ch_eslot[d + 1]; e++) {
                const int j = ecam[e];
                if (gcam_of[j] < 0) {
                    gcam_of[j] = (int)ge.size();
                    ge.push_back(j);
                }
                P.ce_g[e] = (unsigned short)gcam_of[j];
            }
            if ((int)gs.size() > gs_cap) {   // direct group: this chunk alone
                d++;
                break;
            }
        }
        for (int b : gs) {
            P.gslot_blk.push_back(b);
            gslot_of[b] = -1;
        }
        for (int j : ge) {
            P.gecam.push_back(j);
            gcam_of[j] = -1;
        }
        if (mf) {
            P.mf_max_s = std::max(P.mf_max_s, (int)gs.size());
            P.mf_max_e = std::max(P.mf_max_e, (int)ge.size());
            P.ngrp_mf++;
        } else if ((int)gs.size() <= gs_cap) {   // LDS accumulators actually needed
            P.grp_max_s = std::max(P.grp_max_s, (int)gs.size());
            P.grp_max_e = std::max(P.grp_max_e, (int)ge.size());
        }
        P.grp_ch.push_back(d);
        P.grp_gs.push_back((int)P.gslot_blk.size());
        P.grp_ge.push_back((int)P.gecam.size());
        c = d;
    }
    PLAN_T("groups");
    // long tracks' Schur terms (no slots of their own): k_schur_reduce adds,
    // per block (j, k), the terms Y_a W_b^T of every long track that sees both
    // cameras, in track order, by merging the two cameras' lists of long-track
    // observations (cam_lptr / cam_lobs / cam_ltrk: per camera its long-track
    // observations in ascending order = track order; a point sees a camera at
    // most once).  One group e-slot per long observation (its Y_a eB_i term,
    // k_long_y), after the regular ones.
    const int nlong = (int)P.long_pt.size();
    const int L0 = nlong ? P.long_o0[0] : 0, nlobs = nlong ? P.long_o0[nlong] - L0 : 0;
    for (int l = 0; l < nlong; l++)
        P.long_ebase.push_back((int)P.gecam.size() + (P.long_o0[l] - L0));
    P.gecam.insert(P.gecam.end(), lcam.begin() + L0, lcam.begin() + L0 + nlobs);
    {
        P.cam_lptr.assign(m + 1, 0);
        for (int o = L0; o < L0 + nlobs; o++) P.cam_lptr[lcam[o] + 1]++;
        for (int j = 0; j < m; j++) P.cam_lptr[j + 1] += P.cam_lptr[j];
        P.cam_lobs.resize(nlobs);
        P.cam_ltrk.resize(nlobs);
        std::vector<int> pos(P.cam_lptr.begin(), P.cam_lptr.end() - 1);
        for (int l = 0; l < nlong; l++)
            for (int o = P.long_o0[l]; o < P.long_o0[l + 1]; o++) {
                const int q = pos[lcam[o]]++;
                P.cam_lobs[q] = o - L0;
                P.cam_ltrk[q] = l;
            }
        for (int j = 0; j < m; j++)
            P.max_lcam = std::max(P.max_lcam, P.cam_lptr[j + 1] - P.cam_lptr[j]);
    }
    PLAN_T("long lists");
#ifdef BA_PLAN_TIMING
    std::fprintf(stderr, "   (group slots %zu; group e-slots %zu; long tracks %d, %d observations, "
                 "at most %d per camera)\n", P.gslot_blk.size(), P.gecam.size(), nlong, nlobs,
                 P.max_lcam);
#endif
    bucket(P.gslot_blk, nb, P.blk_gptr, P.blk_gslots);
    bucket(P.gecam, m, P.cam_gptr, P.cam_gslots);
    PLAN_T("buckets");
    P.ch_blob.assign(1, 0);
    P.ch_obase.assign(1, lptr[0]);
    if (P.nch_mf > 0) {
        // dense-layout record per chunk (k_schur_mfma):
        //   [np | nobs << 16]
        //   [C | flags << 8 | Kc << 16]  C cameras ascending, Kc = 3 np rounded to 4;
        //        flags: 1 dense (every point sees every camera of the chunk),
        //               2 flush (the next chunk of the group has other cameras, or
        //                 this is the group's last chunk: the register-held MFMA
        //                 tiles and e_ sums go to the group accumulators)
        //   ge[C]       group e-slot of each camera slot
        //   pair[C(C+1)/2]  group slot of block (cam[cr], cam[cc]), cr >= cc, index
        //                   cr (cr + 1) / 2 + cc; 0xffffffff: not in the group
        //   idx[ceil(np C / 4)]  byte p C + cs: local observation index of chunk
        //                        point p in camera slot cs, 0xff if p does not see it
        std::vector<int> cslot(m, -1), gsl_of(nb, -1), gel_of(m, -1);
        std::vector<int> ch_grp(nch);
        for (int g = 0; g + 1 < (int)P.grp_ch.size(); g++)
            for (int c = P.grp_ch[g]; c < P.grp_ch[g + 1]; c++) ch_grp[c] = g;
        auto cams_of = [&](int c, std::vector<int> &cams) {   // (reused buffers)
            cams.assign(ecam.begin() + P.ch_eslot[c], ecam.begin() + P.ch_eslot[c + 1]);
            std::sort(cams.begin(), cams.end());
        };
        std::vector<int> cams, next;
        std::vector<unsigned char> tab;
        cams_of(0, cams);
        for (int c = 0; c < P.nch_mf; c++) {
            const int g = ch_grp[c];
            if (c == P.grp_ch[g]) {   // group-local slot / camera ids
                for (int q = P.grp_gs[g]; q < P.grp_gs[g + 1]; q++)
                    gsl_of[P.gslot_blk[q]] = q - P.grp_gs[g];
                for (int q = P.grp_ge[g]; q < P.grp_ge[g + 1]; q++)
                    gel_of[P.gecam[q]] = q - P.grp_ge[g];
            }
            const int p0 = P.ch_pt[c], p1 = P.ch_pt[c + 1];
            const int nobs = lptr[p1] - lptr[p0];
            const int C = (int)cams.size();
            bool flush = true;
            next.clear();
            if (c + 1 < P.nch_mf) {
                cams_of(c + 1, next);
                flush = ch_grp[c + 1] != g || next != cams;
            }
            for (int q = 0; q < C; q++) cslot[cams[q]] = q;
            const bool dense = nobs == (p1 - p0) * C;
            std::vector<unsigned> &B = P.blob;
            const int kc = (3 * (p1 - p0) + 3) & ~3;
            B.push_back((unsigned)(p1 - p0) | ((unsigned)nobs << 16));
            B.push_back((unsigned)C | ((unsigned)(dense ? 1 : 0) << 8) |
                        ((unsigned)(flush ? 2 : 0) << 8) | ((unsigned)kc << 16));
            for (int q = 0; q < C; q++) B.push_back((unsigned)gel_of[cams[q]]);
            for (int cr = 0; cr < C; cr++)
                for (int cc = 0; cc <= cr; cc++) {
                    const int blk = hb.find(cams[cr], cams[cc]);
                    const int sl = blk >= 0 ? gsl_of[blk] : -1;
                    B.push_back(sl >= 0 ? (unsigned)sl : 0xffffffffu);
                }
            {
                tab.assign((size_t)(p1 - p0) * C, 0xff);
                for (int i = p0; i < p1; i++)
                    for (int o = lptr[i]; o < lptr[i + 1]; o++)
                        tab[(size_t)(i - p0) * C + cslot[lcam[o]]] =
                            (unsigned char)(o - lptr[p0]);
                for (size_t q = 0; q < tab.size(); q += 4) {
                    unsigned w = 0;
                    for (size_t u = 0; u < 4; u++)
                        w |= (unsigned)(q + u < tab.size() ? tab[q + u] : 0xff) << (8 * u);
                    B.push_back(w);
                }
            }
            for (int q = 0; q < C; q++) cslot[cams[q]] = -1;
            if (c + 1 == P.grp_ch[g + 1]) {
                for (int q = P.grp_gs[g]; q < P.grp_gs[g + 1]; q++) gsl_of[P.gslot_blk[q]] = -1;
                for (int q = P.grp_ge[g]; q < P.grp_ge[g + 1]; q++) gel_of[P.gecam[q]] = -1;
            }
            P.ch_blob.push_back((int)B.size());
            P.ch_obase.push_back(lptr[p1]);
            cams.swap(next);
        }
        for (int g = 0; g < P.ngrp_mf; g++)
            P.mf_max_blob = std::max(P.mf_max_blob,
                                     P.ch_blob[P.grp_ch[g + 1]] - P.ch_blob[P.grp_ch[g]]);
    }
    {   // term-chunk records: sizes first, then filled in parallel at their offsets
        const int nt = nch - P.nch_mf;
        std::vector<long long> boff(nt + 1, 0);
        for (int c = P.nch_mf; c < nch; c++) {
            const int s0 = P.ch_slot[c], s1 = P.ch_slot[c + 1];
            const int e0 = P.ch_eslot[c], e1 = P.ch_eslot[c + 1];
            const long long sz = 4 + (s1 - s0 + 1) + (e1 - e0 + 1) + (s1 - s0) + (e1 - e0) +
                                 (lptr[P.ch_pt[c + 1]] - lptr[P.ch_pt[c]]) +
                                 (P.slot_tptr[s1] - P.slot_tptr[s0]) +
                                 (P.eslot_optr[e1] - P.eslot_optr[e0]);
            boff[c - P.nch_mf + 1] = boff[c - P.nch_mf] + sz;
            P.ch_blob.push_back(P.ch_blob.back() + (int)sz);
            P.ch_obase.push_back(lptr[P.ch_pt[c + 1]]);
            P.max_blob = std::max(P.max_blob, (int)sz);
        }
        const size_t bbase = P.blob.size();
        P.blob.resize(bbase + boff[nt]);
        parallel_ranges(nt, plan_threads(boff[nt], 100000), [&](int, int c0, int c1) {
            for (int c = P.nch_mf + c0; c < P.nch_mf + c1; c++) {
                const int p0 = P.ch_pt[c], p1 = P.ch_pt[c + 1];
                const int nobs = lptr[p1] - lptr[p0];
                const int s0 = P.ch_slot[c], s1 = P.ch_slot[c + 1];
                const int e0 = P.ch_eslot[c], e1 = P.ch_eslot[c + 1];
                const int t0 = P.slot_tptr[s0], t1 = P.slot_tptr[s1];
                const int u0 = P.eslot_optr[e0], u1 = P.eslot_optr[e1];
                unsigned *B = &P.blob[bbase + boff[c - P.nch_mf]];
                *B++ = (unsigned)(p1 - p0) | ((unsigned)nobs << 16);
                *B++ = (unsigned)(s1 - s0) | ((unsigned)(e1 - e0) << 16);
                *B++ = (unsigned)(t1 - t0);
                *B++ = (unsigned)(u1 - u0);
                for (int s = s0; s <= s1; s++) *B++ = (unsigned)(P.slot_tptr[s] - t0);
                for (int e = e0; e <= e1; e++) *B++ = (unsigned)(P.eslot_optr[e] - u0);
                for (int s = s0; s < s1; s++) *B++ = P.cs_g[s];
                for (int e = e0; e < e1; e++) *B++ = P.ce_g[e];
                for (int i = p0; i < p1; i++)
                    for (int o = lptr[i]; o < lptr[i + 1]; o++) *B++ = (unsigned)(i - p0);
                for (int t = t0; t < t1; t++)
                    *B++ = (unsigned)P.slot_term[2 * t] | ((unsigned)P.slot_term[2 * t + 1] << 16);
                for (int u = u0; u < u1; u++) *B++ = P.eslot_obs[u];
            }
        }, &boff);
    }
    PLAN_T("blobs");
    for (size_t l = 0; l < P.long_pt.size(); l++)   // segment chunks: no Schur record
        for (int o = P.long_o0[l]; o < P.long_o0[l + 1]; o += BA_CH_OBS) {
            P.ch_blob.push_back(P.ch_blob.back());
            P.ch_obase.push_back(std::min(o + BA_CH_OBS, P.long_o0[l + 1]));
        }
    return true;
}
}  // namespace

// Fast-path point order by track kind (stable within a kind): short tracks
// (<= BA_MF_CMAX(na) views: MFMA Schur chunks) first, then tracks that fit a
// per-term chunk, then long tracks (split into chunk-sized segments with the
// dedicated long-track kernels), so that every kind is one contiguous range.
// Applied when more than one kind is present and no track exceeds the
// long-track caps (else the ordered kernels take the problem).  The
// summation order of the fast path changes with it (it is not the parity
// path); set / get_params and the getters map back to the input order.
int track_kind(long long k, int cmax)
{
    if (k <= cmax) return 0;                                      // MFMA Schur chunk
    if (k <= BA_CH_OBS && k * (k + 1) / 2 <= BA_CH_TERMS) return 1;   // per-term chunk
    return 2;                                                     // long track
}

void order_points_by_kind(int cmax, host_obs &h, std::vector<int> &pt_ptr, int p0, int p1,
                          std::vector<int> &pperm, std::vector<int> &operm)
{
    // points [p0, p1) of the global point-major arrays (this rank's range);
    // pperm / operm are relative to p0 / the range's first observation
    const int n = p1 - p0;
    int cnt[3] = {0, 0, 0};
    long long lterms = 0;
    for (int i = p0; i < p1; i++) {
        const long long k = pt_ptr[i + 1] - pt_ptr[i];
        const int kind = track_kind(k, cmax);
        cnt[kind]++;
        if (kind == 2) {
            if (k > BA_LONG_OBS) return;                          // ordered kernels
            lterms += k * (k + 1) / 2;
        }
    }
    if (lterms > BA_LONG_TERMS) return;
    if ((cnt[0] == 0) + (cnt[1] == 0) + (cnt[2] == 0) >= 2) return;   // one kind: as is
    // stable placement by kind (one counting pass instead of three scans)
    pperm.assign(n, 0);
    {
        int at[3] = {0, cnt[0], cnt[0] + cnt[1]};
        for (int i = 0; i < n; i++) pperm[at[track_kind(pt_ptr[p0 + i + 1] - pt_ptr[p0 + i], cmax)]++] = i;
    }
    const int o0 = pt_ptr[p0];
    const size_t N = (size_t)(pt_ptr[p1] - o0);
    std::vector<int> cam2(N);
    std::vector<double> x2(2 * N);
    operm.resize(N);
    std::vector<int> ptr2(n + 1, 0);
    size_t q = 0;
    for (int i2 = 0; i2 < n; i2++) {
        const int i = p0 + pperm[i2];
        for (int o = pt_ptr[i]; o < pt_ptr[i + 1]; o++, q++) {
            cam2[q] = h.cam[o];
            x2[2 * q] = h.x[2 * (size_t)o];
            x2[2 * q + 1] = h.x[2 * (size_t)o + 1];
            operm[q] = o - o0;
        }
        ptr2[i2 + 1] = (int)q;
    }
    if (o0 == 0 && N == h.cam.size()) {   // the whole list (one rank): swap, no copy back
        h.cam.swap(cam2);
        h.x.swap(x2);
    } else {
        std::copy(cam2.begin(), cam2.end(), h.cam.begin() + o0);
        std::copy(x2.begin(), x2.end(), h.x.begin() + 2 * (size_t)o0);
    }
    for (int i2 = 0; i2 < n; i2++) {
        pt_ptr[p0 + i2 + 1] = o0 + ptr2[i2 + 1];
        for (int o = ptr2[i2]; o < ptr2[i2 + 1]; o++) h.pt[o0 + o] = p0 + i2;
    }
}

// The host side of a context's plan (ctx_setup; tools/bench_plan.cpp times it
// on the CPU): the co-visible block set and, on the fast path, the chunk /
// group plan.  fast is cleared when some track fits no chunk kind (the
// ordered kernels take the problem; hb then carries their term lists).
void plan_host(int m, int na, int n, const std::vector<int> &lptr, const std::vector<int> &lcam,
               const std::vector<int> &pt_ptr_all, const std::vector<int> &cam_all, int p0,
               int p1, long long o0, bool lower_blocks, bool all_diag, bool no_mfma, bool &fast,
               int &p_long, host_blocks &hb, host_plan &plan, void (*mark)(const char *))
{
    // long tracks (more than a chunk holds) must form the tail [p_long, n) of
    // the local points (order_points_by_kind) and stay within the caps; else
    // the sequential kernels take the problem
    p_long = n;
    if (fast) {
        while (p_long > 0 && track_kind(lptr[p_long] - lptr[p_long - 1], BA_MF_CMAX(na)) == 2)
            p_long--;
        long long lterms = 0;
        for (int i = 0; fast && i < n; i++) {
            const long long k = lptr[i + 1] - lptr[i];
            const bool lng = track_kind(k, BA_MF_CMAX(na)) == 2;
            if (lng != (i >= p_long) || k > BA_LONG_OBS) fast = false;
            if (lng) lterms += k * (k + 1) / 2;
        }
        if (lterms > BA_LONG_TERMS) fast = false;
    }
    build_blocks(m, pt_ptr_all, cam_all, p0, p1, o0, lower_blocks, all_diag, !fast, hb);
    if (mark) mark("blocks");
    // MFMA Schur chunks for the leading points whose tracks fit the dense slab
    // (ctx_create orders the short-track points first), per-term chunks for
    // the rest; the ordered kernels if some track fits neither
    if (fast) {
        int p_split = 0;
        if (!no_mfma)
            while (p_split < p_long && lptr[p_split + 1] - lptr[p_split] <= BA_MF_CMAX(na))
                p_split++;
        if (!build_plan(m, na, lptr, lcam, hb, plan, BA_MF_CMAX(na), p_split, p_long)) {
            fast = false;
            hb = host_blocks();
            build_blocks(m, pt_ptr_all, cam_all, p0, p1, o0, lower_blocks, all_diag, true, hb);
        }
    }
}
bool plan_mfma_groups_tile_points(const host_plan &plan, int n)
{
    // the MFMA groups are the only Schur groups and their point ranges, each
    // the chunks ch_pt[grp_ch[g]] .. ch_pt[grp_ch[g + 1]], follow one another
    // from point 0 to point n
    const int ngrp = (int)plan.grp_ch.size() - 1;
    bool tile = plan.ngrp_mf > 0 && ngrp == plan.ngrp_mf && plan.long_pt.empty();
    int at = 0;
    for (int g = 0; tile && g < plan.ngrp_mf; g++) {
        tile = plan.ch_pt[plan.grp_ch[g]] == at &&
               plan.ch_pt[plan.grp_ch[g + 1]] >= at;
        at = plan.ch_pt[plan.grp_ch[g + 1]];
    }
    return tile && at == n;
}

void plan_obs_local_point(const host_plan &plan, const std::vector<int> &lptr,
                          std::vector<unsigned char> &lpt)
{
    lpt.assign(std::max(lptr.back(), 1), 0);
    for (size_t ch = 0; ch + 1 < plan.ch_pt.size(); ch++)
        for (int i = plan.ch_pt[ch]; i < plan.ch_pt[ch + 1]; i++)
            for (int o = lptr[i]; o < lptr[i + 1]; o++)
                lpt[o] = (unsigned char)(i - plan.ch_pt[ch]);
}

void plan_chunk_cameras(const host_plan &plan, const std::vector<int> &lcam,
                        std::vector<int> &ccam)
{
    const size_t nchk = plan.ch_obase.size() - 1;
    ccam.assign(2 * std::max<size_t>(nchk, 1), 0);
    for (size_t ch = 0; ch < nchk; ch++) {
        int lo = INT_MAX, hi = -1;
        for (int o = plan.ch_obase[ch]; o < plan.ch_obase[ch + 1]; o++) {
            lo = std::min(lo, lcam[o]);
            hi = std::max(hi, lcam[o]);
        }
        ccam[2 * ch] = hi < 0 ? 0 : lo;
        ccam[2 * ch + 1] = hi < 0 ? 0 : hi;
    }
}
