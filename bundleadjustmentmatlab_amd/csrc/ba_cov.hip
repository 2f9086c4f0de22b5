// ba_cov.hip -- posterior covariances (vlgba_covariance): the kernels after the
// dense inverse of the undamped reduced camera system.
//
//   Sigma_a   = S0^-1 (rocSOLVER dpotrf + dpotri on the lower triangle; the
//               exactly-zero rows of S0 get the unit diagonal of k_fix_diag and
//               are zeroed again afterwards: k_cov_mark_fixed / k_cov_finish)
//   Sigma_b_i = V+_i + V+_i T_i V+_i,
//   T_i       = sum_{j,k in cams(i)} W_ij^T Sigma_a[j,k] W_ik      (k_point_cov)
//
// The selected method (VLGBA_COV_SELECTED) forms Sigma_a only on the co-visible
// pattern, in the tiles of the cyclic reduction's selected inverse
// (k_cr32_selinv, ba_chol.hip); here are its fixed-row mask from the blocks
// (k_cov_mark_fixed_blocks) and the extraction of the diagonal and packed
// co-visible blocks from those tiles (k_cov_extract).  k_point_cov is the same.
//
// k_point_cov is one streaming pass over the observations, point-major like
// the Schur kernels: a point's W rows (NA x 3 each) are staged in LDS once and
// read by every camera pair of its track.  Sigma_a[k,j] = Sigma_a[j,k]^T, so
// only the pairs j >= k are visited: with M = W_ij^T Sigma_a[j,k] W_ik a pair
// j > k adds M + M^T and a pair j == k adds M, and only the six lower entries
// of T_i are accumulated (the upper ones are their mirror: the result is
// symmetric by construction).
//
// Summation order (fixed: a call repeated on the same state is bit-identical,
// no atomics).  A point is worked on by LPP lanes; pair p = j (j + 1) / 2 + k
// goes to lane p mod LPP, which adds its pairs in ascending p; the lanes'
// partial sums are added by an xor butterfly inside the wave (and, for
// LPP = 256, the four waves' sums in wave order).  Inside a pair every sum
// runs in ascending index order, each term added by an explicit fma (one
// rounding where a product and a sum would have two; the library is otherwise
// built without contraction).  The longest chain of fp64 roundings behind an
// entry is therefore at most
//     2 NA + ceil(pairs / LPP) + log2(LPP) + 10
// (2 NA counts the products and the sums separately; tests/cov_ref.py derives
// its per-entry bound from this with LPP = 8, which covers the three
// instances).
//
// Points are binned by track length (ba_solver.cpp, once per context): up to
// BA_COV_T8 views -> 8 lanes per point, up to BA_COV_T64 -> one wave, longer
// -> one workgroup per point (a track of 140 views has 9,870 pairs: 39 per
// thread), so no wave waits on a long track while its neighbours idle.
//
// Sigma_a[j,k] is read from a packed copy of the co-visible blocks (PK = true:
// block (j, k), k <= j, found by bisection in row j of a CSR index; NA x NA
// contiguous doubles, so an even NA loads a column as 16-byte vectors) or
// straight from the dense inverse (PK = false: columns ld doubles apart).  The
// values are the same, hence so are the results, bit for bit.  cfg3 (tracks of
// 6, 10.5 M pairs): 394 us packed, 400 us dense (profiles/cov_time_cfg3.txt).
#include "ba_internal.h"
#include "ba_chol.h"

// One lane's pairs of one point: the six lower entries of its part of T_i.  Wp:
// the point's W rows (LDS or global memory: a call site of its own for each, so
// that the loads are LDS / global loads and not flat ones); cam: its cameras.
template <int NA, int LPP, bool PK>
__device__ __forceinline__ void cov_pairs(const double *__restrict__ Wp,
                                          const int *__restrict__ cam, int t, int l,
                                          const ba_cov_src &src, double acc[6])
{
    constexpr int WS = 3 * NA;
    // pair p = j (j + 1) / 2 + k, k <= j, p = l, l + LPP, ...
    int j = 0, k = l;
    while (k > j) {
        k -= j + 1;
        j++;
    }
    while (j < t) {
        const double *Wj = Wp + (size_t)WS * j, *Wk = Wp + (size_t)WS * k;
        // cameras ascend within a point: block (cam[j], cam[k]) is in the lower part
        const int cj = cam[j], ck = cam[k];
        const double *B;
        if (PK) {
            int lo = src.rowptr[cj], hi = src.rowptr[cj + 1] - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (src.col[mid] < ck)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            B = src.packed + (size_t)NA * NA * lo;
        } else {
            B = src.Sa + (size_t)NA * cj + (size_t)src.ld * NA * ck;
        }
        const size_t cs = PK ? (size_t)NA : (size_t)src.ld;   // column stride
        double G[NA][3];   // Sigma_a[j,k] W_ik
#pragma unroll
        for (int a = 0; a < NA; a++) G[a][0] = G[a][1] = G[a][2] = 0.0;
#pragma unroll
        for (int b = 0; b < NA; b++) {
            const double w0 = Wk[b], w1 = Wk[b + NA], w2 = Wk[b + 2 * NA];
            const double *Bb = B + cs * b;
            if (PK && NA % 2 == 0) Bb = (const double *)__builtin_assume_aligned(Bb, 16);
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const double s = Bb[a];
                G[a][0] = fma(s, w0, G[a][0]);
                G[a][1] = fma(s, w1, G[a][1]);
                G[a][2] = fma(s, w2, G[a][2]);
            }
        }
        double M[3][3];    // W_ij^T (Sigma_a[j,k] W_ik)
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < NA; a++) s = fma(Wj[a + NA * r], G[a][c], s);
                M[r][c] = s;
            }
        if (j == k) {
            acc[0] = acc[0] + M[0][0];
            acc[1] = acc[1] + M[1][0];
            acc[2] = acc[2] + M[2][0];
            acc[3] = acc[3] + M[1][1];
            acc[4] = acc[4] + M[2][1];
            acc[5] = acc[5] + M[2][2];
        } else {
            acc[0] = acc[0] + (M[0][0] + M[0][0]);
            acc[1] = acc[1] + (M[1][0] + M[0][1]);
            acc[2] = acc[2] + (M[2][0] + M[0][2]);
            acc[3] = acc[3] + (M[1][1] + M[1][1]);
            acc[4] = acc[4] + (M[2][1] + M[1][2]);
            acc[5] = acc[5] + (M[2][2] + M[2][2]);
        }
        k += LPP;
        while (k > j) {
            k -= j + 1;
            j++;
        }
    }
}

template <int NA, int LPP, bool PK>
__global__ __launch_bounds__(256) void k_point_cov(
    const int *__restrict__ list, int nlist, const int *__restrict__ pt_ptr,
    const int *__restrict__ obs_cam, const double *__restrict__ W,
    const double *__restrict__ Vinv, const ba_cov_src src, int tcap, double *__restrict__ out)
{
    constexpr int PPB = 256 / LPP;   // points per workgroup
    constexpr int WS = 3 * NA;       // doubles per W_ij
    extern __shared__ __align__(16) double sm[];
    const int g = threadIdx.x / LPP, l = threadIdx.x % LPP;
    const int li = blockIdx.x * PPB + g;
    const bool valid = li < nlist;
    const int i = valid ? list[li] : 0;
    const int o0 = valid ? pt_ptr[i] : 0;
    const int t = valid ? pt_ptr[i + 1] - o0 : 0;
    // the point's W rows: LDS when they fit the group's share (tcap rows)
    const double *Wg = W + (size_t)WS * o0;
    const bool staged = tcap > 0 && t <= tcap;
    if (tcap > 0) {
        double *w = sm + (size_t)g * tcap * WS;
        if (staged)
            for (int q = l; q < t * WS; q += LPP) w[q] = Wg[q];
        __syncthreads();
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // T(0,0) (1,0) (2,0) (1,1) (2,1) (2,2)
    if (staged)
        cov_pairs<NA, LPP, PK>(sm + (size_t)g * tcap * WS, obs_cam + o0, t, l, src, acc);
    else
        cov_pairs<NA, LPP, PK>(Wg, obs_cam + o0, t, l, src, acc);
    // the lanes' partial sums: xor butterfly (every lane ends with the same sum)
    constexpr int WL = LPP < 64 ? LPP : 64;
#pragma unroll
    for (int s = 1; s < WL; s <<= 1)
#pragma unroll
        for (int q = 0; q < 6; q++) acc[q] = acc[q] + __shfl_xor(acc[q], s, WL);
    if (LPP == 256) {   // one point per workgroup: the four waves' sums in wave order
        __syncthreads();   // (the W rows in sm are no longer read)
        if ((threadIdx.x & 63) == 0)
            for (int q = 0; q < 6; q++) sm[6 * (threadIdx.x >> 6) + q] = acc[q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int q = 0; q < 6; q++)
                acc[q] = ((sm[q] + sm[6 + q]) + sm[12 + q]) + sm[18 + q];
    }
    if (l != 0 || !valid) return;
    const double T[3][3] = {{acc[0], acc[1], acc[2]}, {acc[1], acc[3], acc[4]},
                            {acc[2], acc[4], acc[5]}};
    double Vi[3][3];   // V+ [r][c] (column major in memory)
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) Vi[r][c] = Vinv[9 * (size_t)i + r + 3 * c];
    double P[3][3];    // T V+
    for (int s = 0; s < 3; s++)
        for (int c = 0; c < 3; c++)
            P[s][c] = (T[s][0] * Vi[0][c] + T[s][1] * Vi[1][c]) + T[s][2] * Vi[2][c];
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c <= r; c++) {
            const double q = (Vi[r][0] * P[0][c] + Vi[r][1] * P[1][c]) + Vi[r][2] * P[2][c];
            R[r][c] = Vi[r][c] + q;
            R[c][r] = R[r][c];
        }
    double *o = out + 9 * (size_t)i;
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) o[r + 3 * c] = R[r][c];
}

// rows of the dense lower S0 whose diagonal is exactly zero (fixed parameters:
// the rule of k_fix_diag, which runs next and gives them a unit diagonal)
__global__ void k_cov_mark_fixed(const double *__restrict__ S, long long ld,
                                 unsigned char *__restrict__ fixed)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < ld) fixed[r] = S[r + ld * r] == 0.0 ? 1 : 0;
}

// dpotri left the inverse in the lower triangle: zero the fixed rows and
// columns and mirror it (32 x 32 tiles through LDS: both triangles are read and
// written along columns)
__global__ __launch_bounds__(256) void k_cov_finish(double *__restrict__ S, long long ld,
                                                    const unsigned char *__restrict__ fixed)
{
    __shared__ double tile[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;   // tile row / column, bi >= bj
    if (bi < bj) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int q = ty; q < 32; q += 8) {
        const long long r = 32LL * bi + tx, c = 32LL * bj + q;
        double v = 0.0;
        if (r < ld && c < ld && r >= c) {
            v = (fixed[r] || fixed[c]) ? 0.0 : S[r + ld * c];
            S[r + ld * c] = v;
        }
        tile[q][tx] = v;   // tile[c][r]
    }
    __syncthreads();
    for (int q = ty; q < 32; q += 8) {
        // upper entry (row c', column r') = lower entry (r', c')
        const long long cu = 32LL * bj + tx, ru = 32LL * bi + q;   // lower (ru, cu)
        if (ru < ld && cu < ld && ru > cu) S[cu + ld * ru] = tile[tx][q];
    }
}

// the diagonal NA x NA blocks of the finished inverse
__global__ void k_cov_diag(const double *__restrict__ S, long long ld, int na, int m,
                           double *__restrict__ blocks)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nn = (long long)na * na;
    if (q >= nn * m) return;
    const long long j = q / nn, e = q % nn, r = e % na, c = e / na;
    blocks[q] = S[(na * j + r) + ld * (na * j + c)];
}

// the co-visible blocks (bj[p], bk[p]), bk <= bj, of the finished inverse, packed
__global__ void k_cov_pack(const double *__restrict__ S, long long ld, int na,
                           const int *__restrict__ bj, const int *__restrict__ bk, int nb,
                           double *__restrict__ packed)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nn = (long long)na * na;
    if (q >= nn * nb) return;
    const long long p = q / nn, e = q % nn, r = e % na, c = e / na;
    packed[q] = S[((long long)na * bj[p] + r) + ld * ((long long)na * bk[p] + c)];
}

// ---- the selected method (VLGBA_COV_SELECTED): Sigma_a on the tile-tridiagonal
// pattern of S0, in the tiles of the CR's selected inverse (k_cr32_selinv,
// ba_chol.hip) ----
// the fixed rows from the co-visible blocks (fixed preset to 1: a camera
// without a diagonal block has an all-zero row)
__global__ void k_cov_mark_fixed_blocks(const int *__restrict__ blk_jk,
                                        const double *__restrict__ sblk, int nb, int na,
                                        unsigned char *__restrict__ fixed)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)nb * na) return;
    const long long p = q / na;
    const int r = (int)(q % na), j = blk_jk[2 * p];
    if (j != blk_jk[2 * p + 1]) return;
    fixed[(long long)na * j + r] = sblk[(long long)na * na * p + r + na * r] == 0.0 ? 1 : 0;
}

// Entry q < na^2 nb: entry (r, c) of packed block p = (bj[p], bk[p]), bj >= bk;
// then na^2 m more: the diagonal blocks.  Camera j lives in tile j / G at rows
// na (j % G) (G = TB / na cameras a tile).  Same tile: Sigma_ee of the tile;
// adjacent tiles (tj = tk + 1): the even one was eliminated at level 0 with the
// other as its neighbour -- Xp[tj] = Sigma(tj, tk) as stored, or Xq[tk] =
// Sigma(tk, tj) transposed.  Rows r >= TB of a tile (padding) are never read.
__global__ void k_cov_extract(const double *__restrict__ sig, int nt, int TB, int na, int m,
                              const unsigned char *__restrict__ fixed,
                              const int *__restrict__ bj, const int *__restrict__ bk, int nb,
                              double *__restrict__ diag, double *__restrict__ packed)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nn = (long long)na * na;
    if (q >= nn * ((long long)nb + m)) return;
    const bool dg = q >= nn * nb;
    const long long p = dg ? (q - nn * nb) / nn : q / nn;
    const int e = (int)(q % nn), r = e % na, c = e / na;
    const int j = dg ? (int)p : bj[p], k = dg ? (int)p : bk[p];
    const int G = TB / na, tj = j / G, tk = k / G;
    const int rj = na * (j % G) + r, ck = na * (k % G) + c;
    const long long T2 = 32 * 32;
    double v = 0.0;
    if (!(fixed[(long long)na * j + r] || fixed[(long long)na * k + c])) {
        if (tj == tk)
            v = sig[T2 * tj + 32 * rj + ck];
        else if (tk & 1)   // tj is even: Xp[tj]
            v = sig[T2 * ((long long)nt + tj) + 32 * rj + ck];
        else               // tk is even: Xq[tk]^T
            v = sig[T2 * (2LL * nt + tk) + 32 * ck + rj];
    }
    (dg ? diag : packed)[dg ? q - nn * nb : q] = v;
}

int ba_cov_mark_fixed_blocks(ba_dev *d, unsigned char *fixed)
{
    if (d->ld <= 0) return 0;
    VLGBA_CHECK(hipMemsetAsync(fixed, 1, (size_t)d->ld, d->stream));
    const long long q = (long long)d->nb * d->na;
    if (q > 0)
        k_cov_mark_fixed_blocks<<<(int)((q + 255) / 256), 256, 0, d->stream>>>(
            d->blk_jk, d->sblk, d->nb, d->na, fixed);
    return -(int)hipGetLastError();
}

int ba_cov_extract(ba_dev *d, const double *sig, const unsigned char *fixed, const int *bj,
                   const int *bk, int nb, double *diag, double *packed)
{
    const long long q = (long long)d->na * d->na * ((long long)nb + d->m);
    if (q > 0)
        k_cov_extract<<<(int)((q + 255) / 256), 256, 0, d->stream>>>(
            sig, d->chol->plan.nt32, d->chol->plan.tb32, d->na, d->m, fixed, bj, bk, nb, diag,
            packed);
    return -(int)hipGetLastError();
}

int ba_cov_pack(ba_dev *d, const double *S, long long ld, const int *bj, const int *bk, int nb,
                double *packed)
{
    const long long q = (long long)d->na * d->na * nb;
    if (q > 0)
        k_cov_pack<<<(int)((q + 255) / 256), 256, 0, d->stream>>>(S, ld, d->na, bj, bk, nb,
                                                                   packed);
    return -(int)hipGetLastError();
}

int ba_cov_mark_fixed(ba_dev *d, const double *S, long long ld, unsigned char *fixed)
{
    if (ld > 0)
        k_cov_mark_fixed<<<(int)((ld + 255) / 256), 256, 0, d->stream>>>(S, ld, fixed);
    return -(int)hipGetLastError();
}

int ba_cov_finish(ba_dev *d, double *S, long long ld, const unsigned char *fixed, double *blocks)
{
    if (ld <= 0) return 0;
    const unsigned nt = (unsigned)((ld + 31) / 32);
    k_cov_finish<<<dim3(nt, nt), 256, 0, d->stream>>>(S, ld, fixed);
    const long long q = (long long)d->na * d->na * d->m;
    k_cov_diag<<<(int)((q + 255) / 256), 256, 0, d->stream>>>(S, ld, d->na, d->m, blocks);
    return -(int)hipGetLastError();
}

template <int NA, int LPP, bool PK>
static int launch_point_cov(ba_dev *d, const int *list, int nlist, int tcap,
                            const ba_cov_src &src, double *out)
{
    if (nlist <= 0) return 0;
    constexpr int PPB = 256 / LPP;
    // W rows of the workgroup's points; LPP = 256 also keeps 24 doubles of wave sums
    size_t bytes = sizeof(double) * (size_t)PPB * tcap * 3 * NA;
    if (LPP == 256 && bytes < sizeof(double) * 24) bytes = sizeof(double) * 24;
    const void *fn = (const void *)k_point_cov<NA, LPP, PK>;
    TRY_RC(ba_ensure_dyn_lds(fn, bytes));
    k_point_cov<NA, LPP, PK><<<(nlist + PPB - 1) / PPB, 256, bytes, d->stream>>>(
        list, nlist, d->pt_ptr, d->obs_cam, d->W, d->Vinv, src, tcap, out);
    return -(int)hipGetLastError();
}

template <int NA, bool PK>
static int point_cov_all(ba_dev *d, const int *list, int n8, int n64, int nwg, int tmax,
                         const ba_cov_src &src, double *out)
{
    TRY_RC((launch_point_cov<NA, 8, PK>(d, list, n8, BA_COV_T8, src, out)));
    TRY_RC((launch_point_cov<NA, 64, PK>(d, list + n8, n64, BA_COV_T64, src, out)));
    // a long track's rows in LDS while they fit BA_COV_LDS bytes, else read from
    // global memory (L2) by every pair
    const size_t need = sizeof(double) * (size_t)tmax * 3 * NA;
    return launch_point_cov<NA, 256, PK>(d, list + n8 + n64, nwg,
                                         need <= BA_COV_LDS ? tmax : 0, src, out);
}

template <int NA>
static int point_cov_src(ba_dev *d, const int *list, int n8, int n64, int nwg, int tmax,
                         const ba_cov_src &src, double *out)
{
    return src.packed ? point_cov_all<NA, true>(d, list, n8, n64, nwg, tmax, src, out)
                      : point_cov_all<NA, false>(d, list, n8, n64, nwg, tmax, src, out);
}

int ba_launch_point_cov(ba_dev *d, const int *list, int n8, int n64, int nwg, int tmax,
                        const ba_cov_src *src, double *out)
{
    switch (d->na) {
    case 6: return point_cov_src<6>(d, list, n8, n64, nwg, tmax, *src, out);
    case 7: return point_cov_src<7>(d, list, n8, n64, nwg, tmax, *src, out);
    case BA_RAD_NA: return point_cov_src<BA_RAD_NA>(d, list, n8, n64, nwg, tmax, *src, out);
    case 10: return point_cov_src<10>(d, list, n8, n64, nwg, tmax, *src, out);
    case BA_PROJ_NA: return point_cov_src<BA_PROJ_NA>(d, list, n8, n64, nwg, tmax, *src, out);
    default: return -1000;
    }
}
