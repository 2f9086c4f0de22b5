// ba_pcg.hip -- block-Jacobi preconditioned conjugate gradients on the reduced
// camera system (dense_solve = 5; state: ba_pcg.h).
//
// S da = e_ from da = 0, on the co-visible blocks the Schur phase leaves in
// sblk (j >= k, column major; a diagonal block's lower triangle) and rhs: no
// dense S.  The structure is a block CSR over both triangles (pcg_plan,
// ba_chol_plan.cpp): row j lists its neighbours k ascending, each a block index
// and whether the row reads the block transposed -- an index expression, not a
// copy.  M_j is camera j's diagonal block; its inverse is formed once per pass.
//
//   k_pcg_precond   per camera: the zero-row rule, Cholesky of M_j, M_j^-1,
//                   da = 0, r = e_, z = p = M^-1 r, partials of r'z
//   k_pcg_init      one workgroup: rz_0, the state words, the status word
//   per iteration k (three launches, the iteration number an argument):
//   k_pcg_product   q = S p (one wave per camera row) and the partials of p'q
//   k_pcg_update    alpha = rz / p'q; da += alpha p; r -= alpha q; z = M^-1 r;
//                   the partials of r'z
//   k_pcg_direction beta = rz' / rz; p = z + beta p; workgroup 0 writes rz',
//                   the iteration count, sqrt(rz' / rz_0) and the done word
//
// Scalars stay on the device.  A launch of iteration k reads done[k & 1] and
// returns at once when it is set; only k_pcg_direction writes a done word, the
// other one (done[(k + 1) & 1]), so no word is read and written by the same
// launch.  The host enqueues iterations in batches (BA_PCG_BATCH0, doubling
// to BA_PCG_BATCH_MAX) and reads the state once per batch.  No grid barrier, no
// cooperative launch, no hand-off spin, no atomics.
//
// Order of every sum (fixed: two solves of the same system give the same bits
// and the same iteration count).  A row's product: lane (r, s) sums the
// neighbours s, s + NS, ... (NS = 64 / NA slices) ascending, the columns of a
// block ascending; the slices are then added in order 0 .. NS - 1.  A dot
// product: the NA terms of a camera ascending, the BA_PCG_ROWS cameras of a
// workgroup ascending, then wg_sum over the workgroups' partials -- every
// workgroup of the next launch repeats that last sum and gets the same bits.
//
// Exactly-zero rows (a diagonal entry of the diagonal block == 0, or no
// diagonal block: k_fix_diag's rule, ba_cov_mark_fixed_blocks' on blocks): M_j
// gets a unit diagonal there and zeros in the row and column, rhs 0, and q is
// forced to 0 on the row, so r, z, p and da stay exactly 0.
//
// Failure (the status word scal[4] = 1, as a non-positive pivot of the direct
// solves; the pass then takes pinv(S) e_): a non-positive pivot in a diagonal
// block, p'Sp <= 0, or a scalar that is not finite.
#include "ba_internal.h"
#include "ba_pcg.h"
#include "ba_chol_plan.h"
#include "../../include/vlgba.h"

#include <algorithm>
#include <cmath>
#include <vector>

#define ROWS BA_PCG_ROWS

namespace {

// part[0 .. n) summed by the 256 threads of a workgroup in a fixed order:
// thread t takes t, t + 256, ... ascending, then a binary tree in LDS
__device__ double wg_sum(const double *part, int n, double *red)
{
    const int t = threadIdx.x;
    double s = 0.0;
    for (int q = t; q < n; q += 256) s += part[q];
    red[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    const double v = red[0];
    __syncthreads();
    return v;
}

// entry (r, c) of a symmetric NA x NA block kept as its lower triangle
template <int NA>
__device__ __forceinline__ int lower_of(int r, int c)
{
    return r >= c ? r + NA * c : c + NA * r;
}

template <int NA>
__global__ __launch_bounds__(256) void k_pcg_precond(
    const double *__restrict__ sblk, const int *__restrict__ dblk, int m,
    double *__restrict__ rhs, double *__restrict__ minv, unsigned char *__restrict__ fixed,
    double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
    double *__restrict__ p, double *__restrict__ part_fail, double *__restrict__ part_rz)
{
    __shared__ double Ms[ROWS][NA * NA];   // M_j, then its Cholesky factor (lower)
    __shared__ double Is[ROWS][NA * NA];   // M_j^-1, column c by lane c
    __shared__ double rs[ROWS][NA], zs[ROWS][NA];
    __shared__ int fx[ROWS][NA];
    __shared__ double wsum[ROWS][2];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = ROWS * blockIdx.x + w;
    const bool live = j < m;
    const int b = live ? dblk[j] : -1;
    for (int q = lane; q < NA * NA; q += 64)
        Ms[w][q] = b >= 0 ? sblk[(size_t)NA * NA * b + lower_of<NA>(q % NA, q / NA)] : 0.0;
    __syncthreads();
    if (lane < NA) {
        const bool f = Ms[w][lane + NA * lane] == 0.0;
        fx[w][lane] = f;
        double v = 0.0;
        if (live) {
            const size_t i = (size_t)NA * j + lane;
            fixed[i] = f;
            if (f)
                rhs[i] = 0.0;
            else
                v = rhs[i];
            x[i] = 0.0;
            r[i] = v;
        }
        rs[w][lane] = v;
    }
    __syncthreads();
    for (int q = lane; q < NA * NA; q += 64) {
        const int rr = q % NA, c = q / NA;
        if (fx[w][rr] || fx[w][c]) Ms[w][q] = rr == c ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lane == 0) {   // left-looking Cholesky, in place
        double *L = Ms[w];
        int bad = 0;
        for (int c = 0; c < NA && !bad; c++) {
            double dsum = L[c + NA * c];
            for (int k = 0; k < c; k++) dsum -= L[c + NA * k] * L[c + NA * k];
            if (!(dsum > 0.0) || !isfinite(dsum)) {
                bad = 1;
                break;
            }
            const double l = sqrt(dsum);
            L[c + NA * c] = l;
            for (int i = c + 1; i < NA; i++) {
                double s = L[i + NA * c];
                for (int k = 0; k < c; k++) s -= L[i + NA * k] * L[c + NA * k];
                L[i + NA * c] = s / l;
            }
        }
        wsum[w][0] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lane < NA) {   // column `lane` of the inverse: L y = e, L^T u = y
        const double *L = Ms[w];
        double *y = &Is[w][NA * lane];
        if (wsum[w][0] != 0.0) {
            for (int i = 0; i < NA; i++) y[i] = 0.0;
        } else {
            for (int i = 0; i < NA; i++) {
                double s = i == lane ? 1.0 : 0.0;
                for (int k = 0; k < i; k++) s -= L[i + NA * k] * y[k];
                y[i] = s / L[i + NA * i];
            }
            for (int i = NA - 1; i >= 0; i--) {
                double s = y[i];
                for (int k = i + 1; k < NA; k++) s -= L[k + NA * i] * y[k];
                y[i] = s / L[i + NA * i];
            }
        }
    }
    __syncthreads();
    // the lower triangle mirrored: M^-1 exactly symmetric
    if (live)
        for (int q = lane; q < NA * NA; q += 64)
            minv[(size_t)NA * NA * j + q] = Is[w][lower_of<NA>(q % NA, q / NA)];
    if (lane < NA) {
        double s = 0.0;
        for (int c = 0; c < NA; c++) s += Is[w][lower_of<NA>(lane, c)] * rs[w][c];
        if (live) {
            const size_t i = (size_t)NA * j + lane;
            z[i] = s;
            p[i] = s;
        }
        zs[w][lane] = rs[w][lane] * s;
    }
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int c = 0; c < NA; c++) s += zs[w][c];
        wsum[w][1] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = 0.0, s = 0.0;
        for (int q = 0; q < ROWS; q++) {
            f += wsum[q][0];
            s += wsum[q][1];
        }
        part_fail[blockIdx.x] = f;
        part_rz[blockIdx.x] = s;
    }
}

// part: [0, nwg) failed diagonal blocks | [nwg, 2 nwg) r'z per workgroup
__global__ __launch_bounds__(256) void k_pcg_init(const double *__restrict__ part, int nwg,
                                                  ba_pcg_state *__restrict__ st,
                                                  double *__restrict__ status)
{
    __shared__ double red[256];
    const double fail = wg_sum(part, nwg, red);
    const double rz0 = wg_sum(part + nwg, nwg, red);
    if (threadIdx.x == 0) {
        const bool bad = fail != 0.0 || !isfinite(rz0) || rz0 < 0.0;
        st->rz0 = rz0;
        st->rz[0] = st->rz[1] = rz0;
        st->relres = bad || rz0 == 0.0 ? 0.0 : 1.0;
        st->done[0] = st->done[1] = bad || rz0 == 0.0;
        st->iters = 0;
        st->conv = !bad && rz0 == 0.0;
        st->fail = 0;
        status[0] = bad ? 1.0 : 0.0;   // as a non-positive pivot of the direct solves
        status[1] = 0.0;               // (no hand-off spins here)
    }
}

template <int NA>
__global__ __launch_bounds__(256) void k_pcg_product(
    const double *__restrict__ sblk, const int *__restrict__ rowptr, const int *__restrict__ ent,
    const int *__restrict__ nbr, int m, const unsigned char *__restrict__ fixed,
    const double *__restrict__ p, double *__restrict__ qv, double *__restrict__ part_pq,
    const ba_pcg_state *__restrict__ st, int it)
{
    if (st->done[it & 1]) return;
    constexpr int NS = 64 / NA;
    __shared__ double acc[ROWS][NS][NA];
    __shared__ double wsum[ROWS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = ROWS * blockIdx.x + w;
    const bool live = j < m;
    const int rr = lane % NA, s = lane / NA;
    double a = 0.0;
    if (live && s < NS) {
        const int e1 = rowptr[j + 1];
        for (int e = rowptr[j] + s; e < e1; e += NS) {
            const int b = ent[2 * e], t = ent[2 * e + 1], k = nbr[e];
            const double *B = sblk + (size_t)NA * NA * b;
            const double *pk = p + (size_t)NA * k;
            if (k == j) {   // the diagonal block: its lower triangle mirrored
#pragma unroll
                for (int c = 0; c < NA; c++) a += B[lower_of<NA>(rr, c)] * pk[c];
            } else if (t) {   // S_jk = S_kj^T
#pragma unroll
                for (int c = 0; c < NA; c++) a += B[c + NA * rr] * pk[c];
            } else {
#pragma unroll
                for (int c = 0; c < NA; c++) a += B[rr + NA * c] * pk[c];
            }
        }
    }
    if (s < NS) acc[w][s][rr] = a;
    __syncthreads();
    if (lane < NA) {
        double v = 0.0, pv = 0.0;
        for (int u = 0; u < NS; u++) v += acc[w][u][lane];
        if (live) {
            const size_t i = (size_t)NA * j + lane;
            if (fixed[i]) v = 0.0;
            qv[i] = v;
            pv = p[i] * v;
        }
        acc[w][0][lane] = pv;   // (this lane's own column)
    }
    __syncthreads();
    if (lane == 0) {
        double v = 0.0;
        for (int c = 0; c < NA; c++) v += acc[w][0][c];
        wsum[w] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int u = 0; u < ROWS; u++) v += wsum[u];
        part_pq[blockIdx.x] = v;
    }
}

template <int NA>
__global__ __launch_bounds__(256) void k_pcg_update(
    const double *__restrict__ minv, int m, int nwg, double *__restrict__ x,
    double *__restrict__ r, double *__restrict__ z, const double *__restrict__ p,
    const double *__restrict__ qv, const double *__restrict__ part_pq,
    double *__restrict__ part_rz, ba_pcg_state *__restrict__ st, int it)
{
    if (st->done[it & 1]) return;
    __shared__ double red[256];
    __shared__ double rs[ROWS][NA], zs[ROWS][NA];
    __shared__ double wsum[ROWS];
    const double pq = wg_sum(part_pq, nwg, red);
    const double alpha = st->rz[it & 1] / pq;
    if (!(pq > 0.0) || !isfinite(alpha)) {   // every workgroup alike; k_pcg_direction ends the solve
        if (blockIdx.x == 0 && threadIdx.x == 0) st->fail = 1;
        return;
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = ROWS * blockIdx.x + w;
    const bool live = j < m;
    if (lane < NA) {
        double v = 0.0;
        if (live) {
            const size_t i = (size_t)NA * j + lane;
            x[i] = x[i] + alpha * p[i];
            v = r[i] - alpha * qv[i];
            r[i] = v;
        }
        rs[w][lane] = v;
    }
    __syncthreads();
    if (lane < NA) {
        double s = 0.0;
        if (live) {
            const double *Mi = minv + (size_t)NA * NA * j;
            for (int c = 0; c < NA; c++) s += Mi[lane + NA * c] * rs[w][c];
            z[(size_t)NA * j + lane] = s;
        }
        zs[w][lane] = rs[w][lane] * s;
    }
    __syncthreads();
    if (lane == 0) {
        double v = 0.0;
        for (int c = 0; c < NA; c++) v += zs[w][c];
        wsum[w] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int u = 0; u < ROWS; u++) v += wsum[u];
        part_rz[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void k_pcg_direction(
    long long ld, int nwg, const double *__restrict__ z, double *__restrict__ p,
    const double *__restrict__ part_rz, ba_pcg_state *__restrict__ st,
    double *__restrict__ status, double tol, int max_iter, int it)
{
    const int cur = it & 1, nxt = cur ^ 1;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st->done[cur]) {
        if (first) st->done[nxt] = 1;
        return;
    }
    if (st->fail) {   // this iteration's p'Sp (k_pcg_update)
        if (first) {
            status[0] = 1.0;
            st->done[nxt] = 1;
        }
        return;
    }
    __shared__ double red[256];
    const double rzn = wg_sum(part_rz, nwg, red);
    const double beta = rzn / st->rz[cur];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < ld) p[i] = z[i] + beta * p[i];
    if (first) {
        const double rel = sqrt(rzn / st->rz0);
        const bool bad = !isfinite(rzn) || !isfinite(rel);
        st->rz[nxt] = rzn;
        st->relres = rel;
        st->iters = it + 1;
        st->conv = !bad && rel <= tol;
        if (bad) status[0] = 1.0;
        st->done[nxt] = bad || rel <= tol || it + 1 >= max_iter;
    }
}

template <typename T>
int pcg_alloc(ba_pcg *c, T **ptr, size_t count)
{
    TRY_RC(dalloc(ptr, count));
    c->bytes += (long long)(sizeof(T) * count);
    return 0;
}

}   // namespace

// The block CSR on the host (pcg_plan_build), the work vectors, M^-1, the
// partial sums.  bytes = 8 (4 + na) ld + ld + 16 ceil(m / 4) + 64 + 8 m + 4 +
// 24 nb (vlgba.h, vlgba_plan_info [32]): linear in nb, m and ld
int ba_pcg_setup(ba_dev *d, const int *blk_jk, int nb)
{
    pcg_plan P;
    const int nnz = pcg_plan_build(d->m, blk_jk, nb, P);
    if (nnz < 0) return VLGBA_E_ARG;
    ba_pcg *c = d->pcg = new ba_pcg();   // (zeroed: null pointers)
    c->tol = 0.1;
    c->max_iter = 500;
    c->nnz = nnz;
    c->nwg = (d->m + ROWS - 1) / ROWS;
    const size_t ld = (size_t)d->ld, m = (size_t)d->m;
    TRY_RC(pcg_alloc(c, &c->rowptr, m + 1));
    TRY_RC(pcg_alloc(c, &c->dblk, m));
    TRY_RC(pcg_alloc(c, &c->ent, 4 * (size_t)nb));
    TRY_RC(pcg_alloc(c, &c->nbr, 2 * (size_t)nb));
    TRY_RC(pcg_alloc(c, &c->vec, 4 * ld));
    TRY_RC(pcg_alloc(c, &c->minv, (size_t)d->na * ld));
    TRY_RC(pcg_alloc(c, &c->fixed, ld));
    TRY_RC(pcg_alloc(c, &c->part, 2 * (size_t)c->nwg));
    static_assert(sizeof(ba_pcg_state) == 64, "the state block is 64 bytes (vlgba.h's formula)");
    TRY_RC(pcg_alloc(c, &c->st, 1));
    TRY_RC(upload(c->rowptr, P.rowptr.data(), P.rowptr.size(), d->stream));
    TRY_RC(upload(c->dblk, P.dblk.data(), P.dblk.size(), d->stream));
    TRY_RC(upload(c->ent, P.ent.data(), P.ent.size(), d->stream));
    TRY_RC(upload(c->nbr, P.nbr.data(), P.nbr.size(), d->stream));
    VLGBA_CHECK(hipMemsetAsync(c->st, 0, sizeof(ba_pcg_state), d->stream));
    // the padding rows of da past ld are never written by a solve
    VLGBA_CHECK(hipMemsetAsync(d->da, 0, sizeof(double) * (size_t)d->lds, d->stream));
    VLGBA_CHECK(hipStreamSynchronize(d->stream));   // P goes out of scope
    return 0;
}

// also after a setup that returned early, and for a context without the PCG
void ba_pcg_free(ba_dev *d)
{
    ba_pcg *c = d->pcg;
    if (!c) return;
    void *dev[] = {c->rowptr, c->dblk, c->ent, c->nbr, c->vec, c->minv, c->fixed, c->part, c->st};
    for (void *q : dev)
        if (q) ba_dfree(q);
    delete c;
    d->pcg = nullptr;
}

template <int NA>
static int pcg_solve(ba_dev *d)
{
    ba_pcg *c = d->pcg;
    const size_t ld = (size_t)d->ld;
    double *r = c->vec, *z = r + ld, *p = z + ld, *q = p + ld;
    double *part_pq = c->part, *part_rz = c->part + c->nwg;
    const int g = c->nwg, gd = (int)((d->ld + 255) / 256);
    hipStream_t s = d->stream;
    // M^-1, r = e_, z = p = M^-1 r; then rz_0 and the state (the failed blocks'
    // count travels in part_pq, which the first product overwrites)
    KT_B(d);
    k_pcg_precond<NA><<<g, 256, 0, s>>>(d->sblk, c->dblk, d->m, d->rhs, c->minv, c->fixed, d->da,
                                        r, z, p, part_pq, part_rz);
    k_pcg_init<<<1, 256, 0, s>>>(c->part, c->nwg, c->st, d->scal + 4);
    KT_E(d, KT_FACTOR);
    ba_pcg_state h{};
    int it = 0, batch = BA_PCG_BATCH0;
    while (it < c->max_iter) {
        const int end = std::min(c->max_iter, it + batch);
        KT_B(d);
        for (; it < end; it++) {
            k_pcg_product<NA><<<g, 256, 0, s>>>(d->sblk, c->rowptr, c->ent, c->nbr, d->m, c->fixed,
                                                p, q, part_pq, c->st, it);
            k_pcg_update<NA><<<g, 256, 0, s>>>(c->minv, d->m, c->nwg, d->da, r, z, p, q, part_pq,
                                               part_rz, c->st, it);
            k_pcg_direction<<<gd, 256, 0, s>>>(d->ld, c->nwg, z, p, part_rz, c->st, d->scal + 4,
                                               c->tol, c->max_iter, it);
        }
        KT_E(d, KT_BACKWARD);
        VLGBA_CHECK(hipGetLastError());
        VLGBA_CHECK(hipMemcpyAsync(&h, c->st, sizeof h, hipMemcpyDeviceToHost, s));
        VLGBA_CHECK(hipStreamSynchronize(s));
        if (h.done[it & 1]) break;
        batch = std::min(2 * batch, BA_PCG_BATCH_MAX);
    }
    c->iters = h.iters;
    c->relres = h.relres;
    c->conv = h.conv;
    c->total += h.iters;
    return 0;
}

int ba_pcg_solve(ba_dev *d)
{
    int rc = 0;
    BA_DISPATCH(d->na, rc = pcg_solve<NA>(d));
    return rc;
}
