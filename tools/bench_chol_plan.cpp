// The reduced solve's host planner on the CPU (no GPU and no ROCm needed):
// csrc/ba_chol_plan.cpp chol_plan_build / chol_nd_step on the co-visible block
// set of a problem read from a file.  The block set is built as a context
// builds it (csrc/ba_plan.cpp: observation sort, track-kind point order,
// plan_host), then planned for num_a 6, 7, 10, 12 (or --na's) and the solver modes
// 0 (auto) .. 4 on devices of the given compute-unit counts.  One "chol" line each with
// the plan's scalars and three FNV-1a values: "solveplan" (every plan vector
// and scalar), "launchplan" (the stored cr32_fplan and chol_nd_step of every
// step, runner off) and "launchrun" (the same with the runner on).
// tests/test_solve_plan.py pins them, tests/test_plan_sanitize.py runs this
// program under the sanitizers.
//
// usage: bench_chol_plan [--ncu NCU[,NCU...]] [--na NA[,NA...]] [--dump DIR] [--nd-verbose]
//                        problem.bin ...
//   --ncu         default 256 (the MI355X)
//   --na          the camera sizes to plan, 1 .. 32 each; default 6,7,10,12
//   --dump DIR    each plan's vectors as int32 files
//   --nd-verbose  the nested dissection's decision (VLGBA_ND=v) on stderr
// Build (tools/bench_plan.sh), with any C++17 compiler:
//   c++ -O3 -std=c++17 -I include -pthread tools/bench_chol_plan.cpp
//       bundleadjustmentmatlab_amd/csrc/ba_plan.cpp
//       bundleadjustmentmatlab_amd/csrc/ba_chol_plan.cpp -o tools/build/bench_chol_plan
// Input: int32 m, n, N, then int32 obs_pt[N], int32 obs_cam[N].
#include "../bundleadjustmentmatlab_amd/csrc/ba_plan.h"
#include "../bundleadjustmentmatlab_amd/csrc/ba_chol_plan.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct fnv {
    unsigned long long h = 1469598103934665603ULL;
    template <typename T> void add(const std::vector<T> &v)
    {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
        for (size_t q = 0; q < v.size() * sizeof(T); q++) h = (h ^ p[q]) * 1099511628211ULL;
        const unsigned long long n = v.size();
        for (int q = 0; q < 8; q++) h = (h ^ ((n >> (8 * q)) & 0xff)) * 1099511628211ULL;
    }
};
double ms_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

template <typename T> unsigned long long hash_of(const std::vector<T> &v)
{
    fnv f;
    f.add(v);
    return f.h;
}
template <typename S> void add_ints(std::vector<int> &v, const S &s)
{
    static_assert(sizeof(S) % sizeof(int) == 0, "a struct of ints");
    const int *p = reinterpret_cast<const int *>(&s);
    v.insert(v.end(), p, p + sizeof(S) / sizeof(int));
}
int nd_steps(const chol_plan &P)
{
    int n = 0;
    for (int t = 0; t < P.nd_np; t++) n = std::max(n, P.nd_a0[t + 1] - P.nd_a0[t]);
    return n;
}
// every vector of the plan, in the order of "solveplan" (and of --dump)
std::vector<const std::vector<int> *> plan_vectors(const chol_plan &P)
{
    return {&P.tfirst, &P.pan_ptr, &P.pan_list, &P.env,  &P.tptr,  &P.tblk,   &P.elim,
            &P.keep,   &P.eptr,    &P.kptr,     &P.frec, &P.srec,  &P.fptr,   &P.sptr,
            &P.crow,   &P.prow,    &P.rowsrc,   &P.pairs, &P.pptr, &P.rec,    &P.klist};
}
std::vector<long long> plan_scalars(const chol_plan &P)
{
    std::vector<long long> v = {P.nt, P.n_env(), P.cr32, P.tb32, P.nt32, P.cr_nlev,
                                P.asm_direct_ok, P.cr_fused, P.nd_np, P.nd_grouped};
    for (int t = 0; t <= BA_ND_MAX; t++) v.push_back(P.nd_a0[t]);
    for (long long x : {P.slds, (long long)P.nd_npair, (long long)P.nd_nrec,
                        (long long)P.back_one_launch, (long long)P.handoff,
                        (long long)P.env_runner, (long long)P.runner_flags})
        v.push_back(x);
    return v;
}
unsigned long long solveplan_hash(const chol_plan &P)
{
    std::vector<unsigned long long> slots;
    for (const std::vector<int> *v : plan_vectors(P)) slots.push_back(hash_of(*v));
    slots.push_back(hash_of(plan_scalars(P)));
    slots.push_back(hash_of(std::vector<double>{P.fl_factor, P.fl_syrk, P.fl_back}));
    return hash_of(slots);
}
// what ba_chol_solve passes to k_cr32_fused / k_factor_multi
unsigned long long launchplan_hash(const chol_plan &P, bool run)
{
    std::vector<int> v;
    if (P.cr_fused) add_ints(v, P.fplan);
    for (int st = 0; st < nd_steps(P); st++) {
        nd_step S;
        chol_nd_step(P, st, run, &S);
        add_ints(v, S);
    }
    return hash_of(v);
}
// int32: the number of vectors, then per vector its length and its entries
// (the scalars first, then plan_vectors' order, then the blocks (j, k))
int dump_plan(const chol_plan &P, const std::vector<int> &jk, const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return 1;
    std::vector<std::vector<int>> all;
    std::vector<int> sc;
    for (long long x : plan_scalars(P)) sc.push_back((int)x);
    all.push_back(sc);
    for (const std::vector<int> *v : plan_vectors(P)) all.push_back(*v);
    all.push_back(jk);
    const int nv = (int)all.size();
    std::fwrite(&nv, sizeof(int), 1, f);
    for (const std::vector<int> &v : all) {
        const int len = (int)v.size();
        std::fwrite(&len, sizeof(int), 1, f);
        if (len) std::fwrite(v.data(), sizeof(int), len, f);
    }
    return std::fclose(f);
}
struct chol_opts {
    std::vector<int> ncu, na;
    std::string dump;
    bool nd_verbose = false;
};
int chol_plans(const char *file, int m, const std::vector<int> &jk, const chol_opts &o)
{
    std::string stem(file);
    stem = stem.substr(stem.find_last_of('/') + 1);
    stem = stem.substr(0, stem.find_last_of('.'));
    for (int ncu : o.ncu)
        for (int na : o.na)
            for (int mode = 0; mode <= 4; mode++) {
                chol_plan_in in{};
                in.m = m;
                in.na = na;
                in.ld = (long long)na * m;
                in.lds = (in.ld + BA_TILE - 1) / BA_TILE * BA_TILE;
                in.ncu = ncu;
                in.dense_solve = mode;
                in.blk_jk = jk.data();
                in.nb = (int)jk.size() / 2;
                in.opt.cr_fused_allowed = true;
                in.opt.nd_grouped = true;
                in.opt.nd_verbose = o.nd_verbose;
                chol_plan P;
                auto t0 = std::chrono::steady_clock::now();
                if (chol_plan_build(in, P)) return 4;
                const double t_plan = ms_since(t0);
                std::printf("chol %s na=%d mode=%d ncu=%d nt=%d n_env=%d cr_nlev=%d cr32=%d tb32=%d "
                            "cr_fused=%d asm_direct_ok=%d nd_np=%d nsep=%d npair=%d nrec=%d "
                            "one_back=%d handoff=%d ms=%.3f solveplan %016llx launchplan %016llx "
                            "launchrun %016llx\n",
                            stem.c_str(), na, mode, ncu, P.nt, P.n_env(), P.cr_nlev, P.cr32, P.tb32,
                            P.cr_fused, P.asm_direct_ok, P.nd_np,
                            P.nd_np ? P.nt - P.nd_a0[P.nd_np] : 0, P.nd_npair, P.nd_nrec,
                            (int)P.back_one_launch, (int)P.handoff, t_plan, solveplan_hash(P),
                            launchplan_hash(P, false), launchplan_hash(P, true));
                if (!o.dump.empty() &&
                    dump_plan(P, jk, o.dump + "/" + stem + "_na" + std::to_string(na) + "_mode" +
                                     std::to_string(mode) + "_ncu" + std::to_string(ncu) + ".bin"))
                    return 5;
            }
    return 0;
}

// the co-visible blocks (j >= k) of the problem in `file`, in a context's order
int read_blocks(const char *file, int &m, std::vector<int> &jk)
{
    FILE *f = std::fopen(file, "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    m = hdr[0];
    const int n = hdr[1], N = hdr[2], na = 6;
    std::vector<int> opt(N), ocam(N);
    if (std::fread(opt.data(), sizeof(int), N, f) != (size_t)N ||
        std::fread(ocam.data(), sizeof(int), N, f) != (size_t)N)
        return 2;
    std::fclose(f);
    std::vector<double> ox(2 * (size_t)N, 0.0), K(4 * (size_t)m, 1.0);
    vlgba_problem p{};
    p.m = m;
    p.n = n;
    p.num_a = na;
    p.num_obs = N;
    p.obs_pt = opt.data();
    p.obs_cam = ocam.data();
    p.obs_x = ox.data();
    p.K = K.data();
    host_obs h;
    if (sort_obs(&p, h)) return 3;
    std::vector<int> pt_ptr_all(n + 1, 0);
    for (size_t q = 0; q < h.pt.size(); q++) pt_ptr_all[h.pt[q] + 1]++;
    for (int i = 0; i < n; i++) pt_ptr_all[i + 1] += pt_ptr_all[i];
    std::vector<int> pperm, operm;
    order_points_by_kind(BA_MF_CMAX(na), h, pt_ptr_all, 0, n, pperm, operm);
    std::vector<int> lptr(pt_ptr_all), lcam(h.cam);
    bool fast = true;
    int p_long = n;
    host_blocks hb;
    host_plan P;
    plan_host(m, na, n, lptr, lcam, pt_ptr_all, h.cam, 0, n, 0, true, true, false, fast, p_long,
              hb, P);
    jk = hb.jk;
    return 0;
}
}  // namespace

int main(int argc, char **argv)
{
    chol_opts chol;
    std::vector<const char *> files;
    for (int q = 1; q < argc; q++) {
        if (!std::strcmp(argv[q], "--ncu") && q + 1 < argc) {
            for (const char *s = argv[++q]; *s; s += std::strcspn(s, ","), s += *s == ',')
                chol.ncu.push_back(std::max(1, std::atoi(s)));
        } else if (!std::strcmp(argv[q], "--na") && q + 1 < argc) {
            for (const char *s = argv[++q]; *s; s += std::strcspn(s, ","), s += *s == ',')
                chol.na.push_back(std::min(32, std::max(1, std::atoi(s))));
        } else if (!std::strcmp(argv[q], "--dump") && q + 1 < argc) {
            chol.dump = argv[++q];
        } else if (!std::strcmp(argv[q], "--nd-verbose")) {
            chol.nd_verbose = true;
        } else {
            files.push_back(argv[q]);
        }
    }
    if (chol.ncu.empty()) chol.ncu.push_back(256);
    if (chol.na.empty()) chol.na = {6, 7, 10, 12};
    if (files.empty()) {
        std::fprintf(stderr, "usage: bench_chol_plan [--ncu NCU[,NCU...]] [--na NA[,NA...]] "
                             "[--dump DIR] [--nd-verbose] problem.bin ...\n");
        return 2;
    }
    for (const char *file : files) {
        int m = 0;
        std::vector<int> jk;
        if (const int rc = read_blocks(file, m, jk)) return rc;
        if (const int rc = chol_plans(file, m, jk, chol)) return rc;
    }
    return 0;
}
