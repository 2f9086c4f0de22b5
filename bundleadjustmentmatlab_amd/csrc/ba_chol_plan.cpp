// ba_chol_plan.cpp -- the reduced solve's host planner (ba_chol_plan.h): which
// of the solve paths of ba_chol.hip a problem takes and every record, list and
// launch plan that path reads.  Host only; a function of its arguments.
#include "ba_chol_plan.h"
#include "../../include/vlgba.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <utility>

#define NB BA_TILE
#define T32 BA_TILE32

#pragma GCC visibility push(hidden)

// ---- nested dissection of the envelope -----------------------------------
namespace {
struct nd_cost_t {
    int crit, ns, n[BA_ND_MAX];
};

// arcs [bnd[t], bnd[t+1]) of consecutive cameras; camera j of arc t joins the
// separator when it is co-visible with a camera of an earlier arc (minK[j] <
// bnd[t]).  Predicted step chain: the longest arc, the separator's columns,
// and the two SYRK launches between them.
nd_cost_t nd_cost(const std::vector<int> &minK, int na, const int *bnd, int K)
{
    nd_cost_t e{};
    int nsep = 0, mx = 0;
    for (int t = 0; t < K; t++) {
        int cnt = 0;
        for (int j = bnd[t]; j < bnd[t + 1]; j++) {
            if (minK[j] < bnd[t])
                nsep++;
            else
                cnt++;
        }
        e.n[t] = (na * cnt + NB - 1) / NB;
        mx = std::max(mx, e.n[t]);
    }
    e.ns = (na * nsep + NB - 1) / NB;
    e.crit = mx + e.ns + (e.ns > 0 ? 2 : 0);
    return e;
}

// K = 2 .. BA_ND_MAX arcs: equal camera counts, then one boundary at a time
// moved while the predicted chain shortens.  Returns the best K (0: none).
int nd_choose(const std::vector<int> &minK, int m, int na, int *bnd_out, int &crit_out)
{
    int bestK = 0;
    crit_out = INT_MAX;
    for (int K = 2; K <= BA_ND_MAX && K <= m; K++) {
        int bnd[BA_ND_MAX + 1];
        for (int t = 0; t <= K; t++) bnd[t] = (int)((long long)t * m / K);
        nd_cost_t cur = nd_cost(minK, na, bnd, K);
        for (int sweep = 0; sweep < 4; sweep++) {
            bool moved = false;
            for (int t = 1; t < K; t++)
                for (int step = std::max(1, m / (4 * K)); step >= 1; step /= 2)
                    for (int dir = -1; dir <= 1; dir += 2)
                        for (;;) {
                            const int nbd = bnd[t] + dir * step;
                            if (nbd <= bnd[t - 1] || nbd >= bnd[t + 1]) break;
                            const int keep = bnd[t];
                            bnd[t] = nbd;
                            const nd_cost_t c = nd_cost(minK, na, bnd, K);
                            if (c.crit < cur.crit) {
                                cur = c;
                                moved = true;
                            } else {
                                bnd[t] = keep;
                                break;
                            }
                        }
            if (!moved) break;
        }
        if (cur.crit < crit_out) {
            crit_out = cur.crit;
            bestK = K;
            for (int t = 0; t <= K; t++) bnd_out[t] = bnd[t];
        }
    }
    return bestK;
}

std::vector<int> nd_min_cam(int m, const int *blk_jk, int nb)
{
    std::vector<int> minK(m);
    for (int j = 0; j < m; j++) minK[j] = j;
    for (int b = 0; b < nb; b++) {
        const int j = blk_jk[2 * b], k = blk_jk[2 * b + 1];
        if (k < minK[j]) minK[j] = k;
    }
    return minK;
}

// the one-launch CR's block ranges (k_cr32_fused): level 0 in 2 or 3 records a
// tile, levels >= 1 three per fused record + one per survivor, then the back
// records
void cr32_fplan_build(const chol_plan &p, int ncu, cr32_fplan &P)
{
    const int nl = p.cr_nlev, nrec = p.eptr[nl];
    P = cr32_fplan{};
    P.nl = nl;
    P.nrec = nrec;
    P.l0two = 3 * p.eptr[1] > ncu;
    P.b0[0] = 0;
    P.b0[1] = (P.l0two ? 2 : 3) * p.eptr[1];
    for (int l = 1; l < nl; l++) {
        const int nf = p.fptr[l + 1] - p.fptr[l];
        const int ns = p.sptr[l + 1] - p.sptr[l];
        P.fofs[l] = p.fptr[l];
        P.sofs[l] = p.sptr[l];
        P.b0[l + 1] = P.b0[l] + 3 * nf + ns;
    }
    P.sofs[nl] = p.sptr[nl];
    for (int l = 0; l <= nl; l++) P.eofs[l] = p.eptr[l];
}
// the cyclic reduction's records for nt tiles: per level the even positions of
// the active list are eliminated (e, p, q: the kept neighbours, -1 at the ends)
// and the odd ones kept (k, e-, e+, k2: the next kept tile)
void cr_records(int nt, std::vector<int> &elim, std::vector<int> &keep, std::vector<int> &eptr,
                std::vector<int> &kptr)
{
    std::vector<int> act(nt);
    elim.clear();
    keep.clear();
    eptr.assign(1, 0);
    kptr.assign(1, 0);
    for (int i = 0; i < nt; i++) act[i] = i;
    while (!act.empty()) {
        const int len = (int)act.size();
        std::vector<int> next;
        for (int t = 0; t < len; t++) {
            if ((t & 1) == 0) {
                elim.push_back(act[t]);
                elim.push_back(t > 0 ? act[t - 1] : -1);
                elim.push_back(t + 1 < len ? act[t + 1] : -1);
            } else {
                keep.push_back(act[t]);
                keep.push_back(act[t - 1]);
                keep.push_back(t + 1 < len ? act[t + 1] : -1);
                keep.push_back(t + 2 < len ? act[t + 2] : -1);
                next.push_back(act[t]);
            }
        }
        eptr.push_back((int)elim.size() / 3);
        kptr.push_back((int)keep.size() / 4);
        act.swap(next);
    }
}
}   // namespace

#pragma GCC visibility pop

extern "C" __attribute__((visibility("default"))) int
vlgba_debug_nd_plan(int m, int num_a, const int *blk_jk, int nb, int *bnd, int *crit)
{
    if (m < 2 || num_a < 1 || nb < 0 || (nb > 0 && !blk_jk) || !bnd || !crit) return -1;
    for (int b = 0; b < nb; b++)
        if (blk_jk[2 * b] < blk_jk[2 * b + 1] || blk_jk[2 * b + 1] < 0 || blk_jk[2 * b] >= m)
            return -1;
    return nd_choose(nd_min_cam(m, blk_jk, nb), m, num_a, bnd, *crit);
}

#pragma GCC visibility push(hidden)

int chol_selinv_sources(const std::vector<int> &elim, const std::vector<int> &eptr,
                        std::vector<int> &src)
{
    const int nrec = (int)elim.size() / 3, nlev = (int)eptr.size() - 1;
    src.assign(2 * (size_t)nrec, 0);
    if (nlev < 0 || (nrec > 0 && (nlev < 1 || eptr[nlev] != nrec))) return -1;
    int nt = 0;
    for (int i = 0; i < nrec; i++) nt = std::max(nt, elim[3 * i] + 1);
    std::vector<int> rec_of(nt, -1), lev_of(nt, -1);
    for (int l = 0; l < nlev; l++)
        for (int i = eptr[l]; i < eptr[l + 1]; i++) {
            const int e = elim[3 * i];
            if (e < 0 || rec_of[e] >= 0) return -1;
            rec_of[e] = i;
            lev_of[e] = l;
        }
    for (int i = 0; i < nrec; i++) {
        const int e = elim[3 * i], p = elim[3 * i + 1], q = elim[3 * i + 2];
        src[2 * (size_t)i] = -1;
        if (p < 0 || q < 0) continue;
        if (p >= nt || q >= nt || rec_of[p] < 0 || rec_of[q] < 0) return -1;
        if (lev_of[p] <= lev_of[e] || lev_of[q] <= lev_of[e] || lev_of[p] == lev_of[q]) return -1;
        const bool first_p = lev_of[p] < lev_of[q];
        const int s = first_p ? rec_of[p] : rec_of[q];
        // the other tile is the source's neighbour on that side
        if (first_p ? elim[3 * s + 2] != q : elim[3 * s + 1] != p) return -1;
        src[2 * (size_t)i] = s;
        src[2 * (size_t)i + 1] = first_p ? 1 : 0;
    }
    return 0;
}

#pragma GCC visibility pop

extern "C" __attribute__((visibility("default"))) int
vlgba_debug_selinv_plan(int ntiles, int *elim, int *eptr, int *src)
{
    if (ntiles < 1 || !elim || !eptr || !src) return -1;
    std::vector<int> el, keep, ep, kp, sr;
    cr_records(ntiles, el, keep, ep, kp);
    if ((int)el.size() != 3 * ntiles || chol_selinv_sources(el, ep, sr)) return -1;
    std::copy(el.begin(), el.end(), elim);
    std::copy(ep.begin(), ep.end(), eptr);
    std::copy(sr.begin(), sr.end(), src);
    return (int)ep.size() - 1;
}

#pragma GCC visibility push(hidden)

int chol_plan_build(const chol_plan_in &in, chol_plan &out)
{
    out = chol_plan{};
    const int *blk_jk = in.blk_jk;
    const int nb = in.nb, na = in.na, m = in.m;
    int nt = (int)(in.lds / NB);
    out.nt = nt;
    out.tfirst.resize(nt);
    // every lower tile for the measurement mode (1) and the sequential parity
    // solve (3); the envelope otherwise (0 auto, 2 envelope without CR, 4 ND)
    const bool all_tiles = in.dense_solve == 1 || in.dense_solve == 3;
    for (int i = 0; i < nt; i++) out.tfirst[i] = all_tiles ? 0 : i;
    if (!all_tiles)
        for (int b = 0; b < nb; b++) {
            const int j = blk_jk[2 * b], k = blk_jk[2 * b + 1];   // j >= k
            const long long r0 = (long long)na * j, c0 = (long long)na * k;
            for (long long r = r0; r < r0 + na; r++) {
                const int ti = (int)(r / NB);
                const int tk = (int)(c0 / NB);
                if (tk < out.tfirst[ti]) out.tfirst[ti] = tk;
            }
        }
    // cyclic reduction when S is tile-tridiagonal (dense_solve 0 = auto):
    // camera-aligned 32-row tiles when the co-visibility band allows them
    // (every block (j, k) within neighbouring groups of floor(32 / NA)
    // cameras), else the 64-row tiles
    int ntc = nt;
    if (in.dense_solve == 0 && na <= 32) {
        const int G = 32 / na, TB = na * G;
        const int nt32 = (int)((in.ld + TB - 1) / TB);
        bool ok = nt32 > 1;
        for (int b = 0; ok && b < nb; b++) {
            const int dj = blk_jk[2 * b] / G - blk_jk[2 * b + 1] / G;
            if (dj > 1 || dj < -1) ok = false;
        }
        if (ok) {
            out.cr32 = 1;
            out.tb32 = TB;
            out.nt32 = nt32;
            ntc = nt32;
            // direct assembly: every camera pair (j >= k) inside a group of G
            // cameras is a block (the diagonal tiles the CR writes back are then
            // fully rewritten by k_schur_reduce every pass)
            long long inside = 0, want = 0;
            for (int b = 0; b < nb; b++)
                inside += blk_jk[2 * b] / G == blk_jk[2 * b + 1] / G;
            for (int g0 = 0; g0 < m; g0 += G) {
                const long long c = std::min(G, m - g0);
                want += c * (c + 1) / 2;
            }
            out.asm_direct_ok = inside == want;
        }
    }
    bool tridiag = in.dense_solve == 0 && nt > 1;
    for (int i = 1; tridiag && i < nt; i++)
        if (out.tfirst[i] < i - 1) tridiag = false;
    if (out.cr32) tridiag = true;
    if (tridiag) {
        const int nt = ntc;   // the CR tile count (64- or camera-aligned 32-row tiles)
        std::vector<int> &elim = out.elim, &keep = out.keep, &eptr = out.eptr, &kptr = out.kptr;
        cr_records(nt, elim, keep, eptr, kptr);
        out.cr_nlev = (int)eptr.size() - 1;
        {   // the CR's algorithmic flops (chol_plan::fl_factor): per elimination
            // record (e, p, q) the factor + inverse of D_e, y_e and one panel per
            // neighbour; per kept record (k, e-, e+, k2) the update of D_k and r_k
            // by its eliminated neighbours and the fill towards k2; the back
            // substitution's GEMVs
            const double t = out.cr32 ? T32 : NB;
            const double potri = 2.0 * t * t * t / 3.0, gemm = 2.0 * t * t * t, gemv = 2.0 * t * t;
            out.fl_factor = out.fl_syrk = out.fl_back = 0.0;
            for (size_t i = 0; i < elim.size(); i += 3) {
                const double nbr = (elim[i + 1] >= 0) + (elim[i + 2] >= 0);
                out.fl_factor += potri + gemv + nbr * gemm;
                out.fl_back += (nbr + 1) * gemv;
            }
            for (size_t i = 0; i < keep.size(); i += 4) {
                const double nbe = 1 + (keep[i + 2] >= 0);
                out.fl_factor += nbe * (gemm + gemv) + (keep[i + 3] >= 0) * gemm;
            }
        }
        if (out.cr32) {   // the fused levels' records (see k_cr32_level)
            const int nl = out.cr_nlev;
            std::vector<int> &frec = out.frec, &srec = out.srec, &fptr = out.fptr,
                             &sptr = out.sptr;
            fptr.assign(nl + 1, 0);
            sptr.assign(nl + 1, 0);
            std::vector<int> em_of(nt, -1), ep_of(nt, -1);
            for (int L = 1; L < nl; L++) {
                for (int i = kptr[L - 1]; i < kptr[L]; i++) {
                    em_of[keep[4 * i]] = keep[4 * i + 1];
                    ep_of[keep[4 * i]] = keep[4 * i + 2];
                }
                for (int i = eptr[L]; i < eptr[L + 1]; i++) {
                    const int e = elim[3 * i];
                    frec.insert(frec.end(), {e, elim[3 * i + 1], elim[3 * i + 2], em_of[e],
                                             ep_of[e]});
                }
                for (int i = kptr[L]; i < kptr[L + 1]; i++) {
                    const int k = keep[4 * i];
                    srec.insert(srec.end(), {k, em_of[k], ep_of[k]});
                }
                fptr[L + 1] = (int)frec.size() / 5;
                sptr[L + 1] = (int)srec.size() / 3;
            }
            fptr[1] = 0;
            sptr[1] = 0;
            // one-launch CR (k_cr32_fused) unless the options forbid it
            out.cr_fused = in.opt.cr_fused_allowed && nl <= BA_CR_MAXLEV;
            if (out.cr_fused) cr32_fplan_build(out, in.ncu, out.fplan);
        }
    }
    // nested dissection (not for tridiagonal S, which the cyclic reduction takes)
    out.nd_grouped = in.opt.nd_grouped;
    std::vector<int> &crow = out.crow, tpart;   // row of camera j; part of tile (arc t, separator np)
    if (!tridiag && (in.dense_solve == 0 || in.dense_solve == 4) && m >= 2 && nt > 1) {
        const bool off = in.opt.nd_off;
        const std::vector<int> minK = nd_min_cam(m, blk_jk, nb);
        int bnd[BA_ND_MAX + 1], crit = INT_MAX;
        const int K = off && in.dense_solve == 0 ? 0 : nd_choose(minK, m, na, bnd, crit);
        bool take = K > 0 && (in.dense_solve == 4 || (nt >= 8 && 4 * crit <= 3 * nt));
        // setup budget: the separator SYRK's host lists cost
        // O(ns^2 s0) and its partials (pairs + CUs) x 33 KB of device memory --
        // a graph with a wide separator keeps the natural order instead
        long long npair_max = 0, setup_ops = 0;
        if (K > 0) {
            const nd_cost_t c = nd_cost(minK, na, bnd, K);
            long long s0t = 0;
            for (int t = 0; t < K; t++) s0t += c.n[t];
            npair_max = (long long)c.ns * (c.ns + 1) / 2;
            setup_ops = npair_max * s0t;
            if (npair_max > BA_ND_MAX_PAIRS || setup_ops > BA_ND_MAX_SETUP) take = false;
        }
        if (in.opt.nd_verbose)
            std::fprintf(stderr, "[vlgba] nested dissection: natural %d tiles, %d arcs -> chain %d, "
                         "<= %lld separator pairs, %lld setup checks%s\n", nt, K, crit, npair_max,
                         setup_ops, take ? "" : " (not taken)");
        if (take) {
            crow.assign(m, -1);
            long long row = 0;
            for (int t = 0; t < K; t++) {
                out.nd_a0[t] = (int)(row / NB);
                for (int j = bnd[t]; j < bnd[t + 1]; j++)
                    if (minK[j] >= bnd[t]) {
                        crow[j] = (int)row;
                        row += na;
                    }
                row = (row + NB - 1) / NB * NB;
            }
            out.nd_a0[K] = (int)(row / NB);
            for (int t = 0; t < K; t++)
                for (int j = bnd[t]; j < bnd[t + 1]; j++)
                    if (minK[j] < bnd[t]) {
                        crow[j] = (int)row;
                        row += na;
                    }
            row = (row + NB - 1) / NB * NB;
            out.nd_np = K;
            out.slds = row;
            nt = (int)(row / NB);
            out.nt = nt;
            tpart.assign(nt, K);
            for (int t = 0; t < K; t++)
                for (int i = out.nd_a0[t]; i < out.nd_a0[t + 1]; i++) tpart[i] = t;
        }
    }
    const bool nd = out.nd_np > 0;
    const int npart = nd ? out.nd_np + 1 : 1;
    const int s0 = nd ? out.nd_a0[out.nd_np] : nt;
    // first[i][P]: the first envelope tile of row i among the columns of part P
    // (the profile is preserved inside each part: arcs never couple, and the
    // separator block fills in, so it is taken dense)
    std::vector<int> first;
    if (nd) {
        out.tfirst.assign(nt, 0);
        first.assign((size_t)nt * npart, INT_MAX);
        for (int i = 0; i < nt; i++) first[(size_t)i * npart + tpart[i]] = i >= s0 ? s0 : i;
        for (int b = 0; b < nb; b++) {
            long long r0 = crow[blk_jk[2 * b]], c0 = crow[blk_jk[2 * b + 1]];
            if (r0 < c0) std::swap(r0, c0);
            const int tk = (int)(c0 / NB), P = tpart[tk];
            for (long long r = r0; r < r0 + na; r++) {
                int &f = first[(size_t)(r / NB) * npart + P];
                if (tk < f) f = tk;
            }
        }
        for (int i = 0; i < nt; i++) {
            int f = i;
            for (int P = 0; P < npart; P++) f = std::min(f, first[(size_t)i * npart + P]);
            out.tfirst[i] = f;
        }
    } else {
        first.assign(out.tfirst.begin(), out.tfirst.end());
    }
    auto in_env = [&](int i, int k) { return first[(size_t)i * npart + (nd ? tpart[k] : 0)] <= k; };
    std::vector<int> &ptr = out.pan_ptr, &list = out.pan_list, &env = out.env;
    ptr.assign(nt + 1, 0);
    for (int k = 0; k < nt; k++) {
        for (int i = k + 1; i < nt; i++)
            if (in_env(i, k)) list.push_back(i);
        ptr[k + 1] = (int)list.size();
    }
    for (int k = 0; k < nt; k++)
        for (int i = k; i < nt; i++)
            if (in_env(i, k)) {
                env.push_back(i);
                env.push_back(k);
            }
    const int n_env = out.n_env();
    {   // per envelope tile: the co-visible blocks (j >= k) overlapping it
        std::vector<int> tid_of((size_t)nt * nt, -1);
        for (int e = 0; e < n_env; e++) tid_of[(size_t)env[2 * e] * nt + env[2 * e + 1]] = e;
        std::vector<std::vector<int>> lists(n_env);
        for (int b = 0; b < nb; b++) {
            long long r0 = (long long)na * blk_jk[2 * b], c0 = (long long)na * blk_jk[2 * b + 1];
            if (nd) {
                r0 = crow[blk_jk[2 * b]];
                c0 = crow[blk_jk[2 * b + 1]];
                if (r0 < c0) std::swap(r0, c0);
            }
            const int t0 = (int)(r0 / NB), t1 = (int)((r0 + na - 1) / NB);
            const int u0 = (int)(c0 / NB), u1 = (int)((c0 + na - 1) / NB);
            for (int t = t0; t <= t1; t++)
                for (int u = u0; u <= u1 && u <= t; u++) {
                    const int e = tid_of[(size_t)t * nt + u];
                    if (e >= 0) lists[e].push_back(b);
                }
        }
        std::vector<int> &tptr = out.tptr, &tblk = out.tblk;
        tptr.assign(n_env + 1, 0);
        for (int e = 0; e < n_env; e++) {
            tblk.insert(tblk.end(), lists[e].begin(), lists[e].end());
            tptr[e + 1] = (int)tblk.size();
        }
    }
    if (nd) {
        std::vector<int> &rowsrc = out.rowsrc, &prow = out.prow;
        rowsrc.assign(out.slds, -1);
        prow.assign(in.lds, -1);
        for (int j = 0; j < m; j++)
            for (int r = 0; r < na; r++) {
                rowsrc[crow[j] + r] = na * j + r;
                prow[(size_t)na * j + r] = crow[j] + r;
            }
        // separator pairs (i >= j, ascending) and their arc columns, chunked
        std::vector<int> &pairs = out.pairs, &pptr = out.pptr, &rec = out.rec,
                         &klist = out.klist;
        pptr.assign(1, 0);
        std::vector<std::vector<int>> kl;
        long long work = 0;
        for (int i = s0; i < nt; i++)
            for (int j = s0; j <= i; j++) {
                std::vector<int> ks;
                for (int k = 0; k < s0; k++)
                    if (in_env(i, k) && in_env(j, k)) ks.push_back(k);
                if (ks.empty()) continue;
                work += (long long)ks.size();
                pairs.push_back(i);
                pairs.push_back(j);
                kl.push_back(std::move(ks));
            }
        const int kc = (int)std::max<long long>(2, (work + in.ncu - 1) / std::max(1, in.ncu));
        for (size_t p = 0; p < kl.size(); p++) {
            for (size_t q = 0; q < kl[p].size(); q += kc) {
                rec.push_back((int)p);
                rec.push_back((int)klist.size());
                const int cnt = (int)std::min<size_t>(kc, kl[p].size() - q);
                rec.push_back(cnt);
                klist.insert(klist.end(), kl[p].begin() + q, kl[p].begin() + q + cnt);
            }
            pptr.push_back((int)rec.size() / 3);
        }
        out.fl_syrk = (double)work * 2.0 * NB * NB * NB +
                      (double)(pairs.size() / 2) * 2.0 * NB * NB;
        out.nd_npair = (int)pairs.size() / 2;
        out.nd_nrec = (int)rec.size() / 3;
    }
    {   // the envelope's algorithmic flops (see chol_plan::fl_factor; the CR's: above)
        const double t = NB;
        const double potri = 2.0 * t * t * t / 3.0, gemm = 2.0 * t * t * t, gemv = 2.0 * t * t;
        for (int k = 0; k < nt && !out.cr_nlev && in.dense_solve != 3; k++) {
            const double T = ptr[k + 1] - ptr[k];
            // factor + inverse, y_k, T panels and their rhs updates, the trailing
            // pairs of column k (applied in step k + 1; an arc column's separator
            // x separator pairs go to the separator SYRK instead)
            double nsr = 0;
            if (nd && k < s0)
                for (int q = ptr[k]; q < ptr[k + 1]; q++) nsr += list[q] >= s0;
            out.fl_factor += potri + gemv + T * (gemm + gemv) +
                             (T * (T + 1) / 2 - nsr * (nsr + 1) / 2) * gemm;
            out.fl_back += (T + 1) * gemv;
        }
        if (out.cr_nlev > 0 && out.cr_fused) {   // one CR launch: timed as k_cr_factor
            out.fl_factor += out.fl_back;
            out.fl_back = 0.0;
        }
    }
    // the envelope factor's in-launch hand-off, the one-launch backward when
    // every column is co-resident, and runner mode's flags (the runner needs
    // the device panel pointers of the one-launch backward)
    out.handoff = !out.cr_nlev && in.dense_solve != 3;
    out.back_one_launch = out.handoff && nt <= in.ncu;
    out.env_runner = out.handoff && in.opt.env_runner;
    out.runner_flags = out.env_runner && out.back_one_launch;
    return 0;
}

void chol_nd_step(const chol_plan &plan, int st, bool run, nd_step *Pout)
{
    const int np = plan.nd_np, s0 = plan.nd_a0[np];
    const std::vector<int> &pan_ptr = plan.pan_ptr, &pan_list = plan.pan_list;
    nd_step P{};
    P.grouped = plan.nd_grouped;
    int nbk = 0;
    for (int t = 0; t < np; t++) {
        const int k = plan.nd_a0[t] + st;
        if (k >= plan.nd_a0[t + 1]) continue;
        const int p0 = pan_ptr[k], T = pan_ptr[k + 1] - p0;
        const bool cont = k > plan.nd_a0[t];   // not the arc's first column
        const int q0 = cont ? pan_ptr[k - 1] : 0, Tp = cont ? p0 - q0 : 0;
        const int kin = Tp > 0 && pan_list[q0] == k;
        int nsr = 0;   // separator rows among column k-1's trailing rows
        for (int q = q0 + kin; q < q0 + Tp; q++) nsr += pan_list[q] >= s0;
        const int Tr = Tp - kin, u = P.np++;
        P.k[u] = k;
        P.T[u] = T;
        P.Tp[u] = Tp;
        P.pofs[u] = p0;
        P.qofs[u] = q0;
        const int ntr = Tr * (Tr + 1) / 2 - nsr * (nsr + 1) / 2;
        P.ntr[u] = ntr;
        P.kend[u] = run ? plan.nd_a0[t + 1] : 0;
        P.b0[u] = nbk;
        P.pb[u + 1] = P.pb[u] + T;
        nbk += 1 + T;
    }
    // the trailing workgroups: one per trailing pair
    for (int u = 0; u < P.np; u++) {
        P.ts[u] = P.ntr[u];
        P.tb[u + 1] = P.tb[u] + P.ts[u];
    }
    if (!P.grouped) {   // arc-major: arc u's trailing workgroups follow its panels
        int acc = 0;
        for (int u = 0; u < P.np; u++) {
            P.b0[u] = acc;
            acc += 1 + P.T[u] + P.ts[u];
        }
    }
    nbk += P.tb[P.np];
    P.b0[P.np] = nbk;   // the launch's workgroup count
    *Pout = P;
}

#pragma GCC visibility pop

// ---- block-Jacobi PCG (ba_pcg.hip): S as a block CSR over both triangles ----
#pragma GCC visibility push(hidden)

int pcg_plan_build(int m, const int *blk_jk, int nb, pcg_plan &out)
{
    out = pcg_plan{};
    if (m < 1 || nb < 0 || (nb > 0 && !blk_jk)) return -1;
    out.rowptr.assign((size_t)m + 1, 0);
    out.dblk.assign((size_t)m, -1);
    for (int b = 0; b < nb; b++) {
        const int j = blk_jk[2 * b], k = blk_jk[2 * b + 1];
        if (j < k || k < 0 || j >= m) return -1;
        out.rowptr[(size_t)j + 1]++;
        if (j != k) out.rowptr[(size_t)k + 1]++;
    }
    for (int j = 0; j < m; j++) out.rowptr[(size_t)j + 1] += out.rowptr[j];
    const int nnz = out.rowptr[m];
    // (neighbour, block, transposed) per row, then each row by neighbour
    struct ent_t {
        int k, b, t;
    };
    std::vector<ent_t> e((size_t)nnz);
    std::vector<int> fill(out.rowptr.begin(), out.rowptr.end() - 1);
    for (int b = 0; b < nb; b++) {
        const int j = blk_jk[2 * b], k = blk_jk[2 * b + 1];
        e[(size_t)fill[j]++] = {k, b, 0};
        if (j != k) e[(size_t)fill[k]++] = {j, b, 1};
    }
    out.ent.resize(2 * (size_t)nnz);
    out.nbr.resize((size_t)nnz);
    for (int j = 0; j < m; j++) {
        const int e0 = out.rowptr[j], e1 = out.rowptr[(size_t)j + 1];
        std::sort(e.begin() + e0, e.begin() + e1,
                  [](const ent_t &x, const ent_t &y) { return x.k < y.k; });
        for (int q = e0; q < e1; q++) {
            if (q > e0 && e[q].k == e[(size_t)q - 1].k) return -1;   // a pair given twice
            out.ent[2 * (size_t)q] = e[q].b;
            out.ent[2 * (size_t)q + 1] = e[q].t;
            out.nbr[q] = e[q].k;
            if (e[q].k == j) out.dblk[j] = e[q].b;
        }
    }
    return nnz;
}

#pragma GCC visibility pop

extern "C" __attribute__((visibility("default"))) int
vlgba_debug_pcg_plan(int m, const int *blk_jk, int nb, int *rowptr, int *ent)
{
    if (!rowptr || !ent) return -1;
    pcg_plan P;
    const int nnz = pcg_plan_build(m, blk_jk, nb, P);
    if (nnz < 0) return -1;
    std::copy(P.rowptr.begin(), P.rowptr.end(), rowptr);
    std::copy(P.ent.begin(), P.ent.end(), ent);
    return nnz;
}
