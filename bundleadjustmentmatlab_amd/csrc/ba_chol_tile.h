// ba_chol_tile.h -- the device helpers of the reduced solve's kernels
// (ba_chol.hip): the 64-row tile loads / stores, the fp64 MFMA
// (v_mfma_f64_16x16x4_f64) products and the GEMVs on LDS tiles, the lane
// broadcasts, the 16-pivot wave factor and the 64 x 64 factor + inverse built
// on it; the 32-row tile helpers of the camera-aligned cyclic reduction up to
// its 32 x 32 factor (cr32_chol) and the 64 x 64 factor as two of those
// (potrf64_via32).  __device__ __forceinline__ code only: no host code, no
// kernel, so a probe under tools/ can include it alone.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_limits.h"

#define NB 64
static_assert(NB == BA_TILE, "the kernels' tile height is the planner's");
#define LP 66  // LDS row pitch (doubles): conflict-free 16x4 MFMA operand reads

typedef double d4 __attribute__((ext_vector_type(4)));

// S tile (ti, tj) -> LDS row-major T[r][c] (256 threads).  Thread (r = tid&63,
// c0 = tid>>6) moves column c0 + 4u, u = 0..15: each wave reads whole 512-B
// columns (coalesced) and all 16 loads are in flight before the LDS writes.
__device__ __forceinline__ void load_tile(const double *__restrict__ S, long long lds, int ti,
                                          int tj, double *T)
{
    const double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = base[r + lds * (c0 + 4 * u)];
#pragma unroll
    for (int u = 0; u < 16; u++) T[r * LP + c0 + 4 * u] = v[u];
}

// S tile (ti, tj) transposed -> LDS T[c][r] = tile[r][c] (LDS writes contiguous in r)
__device__ __forceinline__ void load_tile_t(const double *__restrict__ S, long long lds, int ti,
                                            int tj, double *T)
{
    const double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = base[r + lds * (c0 + 4 * u)];
#pragma unroll
    for (int u = 0; u < 16; u++) T[(c0 + 4 * u) * LP + r] = v[u];
}

// split forms of load_tile / load_tile_t: fetch to registers, then put, so
// that several tiles' loads can be in flight together
__device__ __forceinline__ void fetch_tile(const double *__restrict__ S, long long lds, int ti,
                                           int tj, double v[16])
{
    const double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = base[r + lds * (c0 + 4 * u)];
}

__device__ __forceinline__ void put_tile(double *T, const double v[16], bool transposed)
{
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        if (transposed)
            T[(c0 + 4 * u) * LP + r] = v[u];
        else
            T[r * LP + c0 + 4 * u] = v[u];
    }
}

typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) unsigned gu32_t;

template <bool SC> __device__ __forceinline__ double ldg(const double *p)
{
    if constexpr (SC)
        return __builtin_bit_cast(
            double, __hip_atomic_load((gu64_t *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    else
        return *p;
}

template <bool SC> __device__ __forceinline__ void stg(double *p, double v)
{
    if constexpr (SC)
        __hip_atomic_store((gu64_t *)p, __builtin_bit_cast(unsigned long long, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// fetch_tile / store_tile with device-coherent (sc1) accesses: tiles handed
// between the envelope runner and the column launches running beside it
__device__ __forceinline__ void fetch_tile_sc(const double *S, long long lds, int ti, int tj,
                                              double v[16])
{
    const double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = ldg<true>(base + r + lds * (c0 + 4 * u));
}

__device__ __forceinline__ void store_tile_sc(double *S, long long lds, int ti, int tj,
                                              const double *T)
{
    double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = T[r * LP + c0 + 4 * u];
#pragma unroll
    for (int u = 0; u < 16; u++) stg<true>(base + r + lds * (c0 + 4 * u), v[u]);
}

// LDS T[r][c] -> row-major 64x64 dst[r*64 + c]
__device__ __forceinline__ void store_rowmajor(double *__restrict__ dst, const double *T)
{
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = T[(r0 + 4 * u) * LP + c];
#pragma unroll
    for (int u = 0; u < 16; u++) dst[(r0 + 4 * u) * NB + c] = v[u];
}

// row-major 64x64 (src[r*64 + c]) -> LDS T[r][c], loads batched as above
__device__ __forceinline__ void load_rowmajor(const double *__restrict__ src, double *T)
{
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = src[(r0 + 4 * u) * NB + c];
#pragma unroll
    for (int u = 0; u < 16; u++) T[(r0 + 4 * u) * LP + c] = v[u];
}

__device__ __forceinline__ void store_tile(double *__restrict__ S, long long lds, int ti, int tj,
                                           const double *T)
{
    double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = T[r * LP + c0 + 4 * u];
#pragma unroll
    for (int u = 0; u < 16; u++) base[r + lds * (c0 + 4 * u)] = v[u];
}

// acc = As[r][:] . Bs[c][:] over K = 64 for the 64x64 tile of a 256-thread WG.
// Wave w owns rows 32*(w>>1) .. +31, cols 32*(w&1) .. +31 as 2x2 MFMA tiles.
// f64 16x16x4 operand map: A lane l -> A[l&15][l>>4], B lane l -> B[l>>4][l&15];
// result register q of lane l -> (row (l>>4) + 4q, col l&15).
__device__ __forceinline__ void mfma_64x64_acc(const double *As, const double *Bs, d4 acc[2][2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * (w >> 1), c0 = 32 * (w & 1);
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll 4
    for (int s = 0; s < NB / 4; s++) {
        const int kk = 4 * s + lk;
        const double a0 = As[(r0 + li) * LP + kk];
        const double a1 = As[(r0 + 16 + li) * LP + kk];
        const double b0 = Bs[(c0 + li) * LP + kk];
        const double b1 = Bs[(c0 + 16 + li) * LP + kk];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void mfma_64x64(const double *As, const double *Bs, d4 acc[2][2])
{
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
    mfma_64x64_acc(As, Bs, acc);
}

// acc = A B^T over K = 64 for A = S tile (ia, kc), B = S tile (jb, kc), the
// operands read straight from S (column-major, L2) in the 16x16x4 operand
// layout instead of from LDS: the same MFMA chain as mfma_64x64 on the
// loaded tiles, bit for bit, without their 64 KB of LDS.
template <bool SCB = false>
__device__ __forceinline__ void mfma_64x64_glb(const double *__restrict__ S, long long lds,
                                               int ia, int jb, int kc, d4 acc[2][2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * (w >> 1), c0 = 32 * (w & 1);
    const int li = lane & 15, lk = lane >> 4;
    const double *A = S + (long long)NB * ia + lds * (long long)NB * kc;
    const double *B = S + (long long)NB * jb + lds * (long long)NB * kc;
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; h++) {   // K in two halves of operand loads
        double a0[8], a1[8], b0[8], b1[8];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const long long kk = lds * (4 * (8 * h + s) + lk);
            a0[s] = A[r0 + li + kk];
            a1[s] = A[r0 + 16 + li + kk];
            b0[s] = ldg<SCB>(B + c0 + li + kk);
            b1[s] = ldg<SCB>(B + c0 + 16 + li + kk);
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b0[s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b1[s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b0[s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b1[s], acc[1][1], 0, 0, 0);
        }
    }
}

// write acc (scale * acc + (add ? T : 0)) into LDS tile T in MFMA layout
__device__ __forceinline__ void acc_to_lds(const d4 acc[2][2], double *T, double scale, bool add)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * (w >> 1), c0 = 32 * (w & 1);
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = r0 + 16 * x + (lane >> 4) + 4 * q, c = c0 + 16 * y + (lane & 15);
                const double v = scale * acc[x][y][q];
                T[r * LP + c] = add ? T[r * LP + c] + v : v;
            }
}

// ---- 16x16 MFMA helpers on LDS row-major tiles (pitch LP), one wave each ----
// nt: acc[r][c] += sum_t A[ra+r][ka+t] * Bt[cb+c][kb+t]   (B given transposed)
// nn: acc[r][c] += sum_t A[ra+r][ka+t] * Bn[kb+t][cb+c]
__device__ __forceinline__ d4 mfma16_nt(const double *A, int ra, int ka, const double *Bt, int cb,
                                        int kb, d4 acc)
{
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(ra + li) * LP + ka + 4 * s + lk],
                                                   Bt[(cb + li) * LP + kb + 4 * s + lk], acc,
                                                   0, 0, 0);
    return acc;
}

__device__ __forceinline__ d4 mfma16_nn(const double *A, int ra, int ka, const double *Bn, int kb,
                                        int cb, d4 acc)
{
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(ra + li) * LP + ka + 4 * s + lk],
                                                   Bn[(kb + 4 * s + lk) * LP + cb + li], acc,
                                                   0, 0, 0);
    return acc;
}

// T[r0 + row][c0 + col] = scale * acc (+ T if add): 16x16 result layout
__device__ __forceinline__ void put16(double *T, int r0, int c0, d4 acc, double scale, bool add)
{
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double *p = T + (r0 + lk + 4 * q) * LP + c0 + li;
        *p = add ? *p + scale * acc[q] : scale * acc[q];
    }
}

// out = scale * M v for a 64x64 LDS tile (row-major, pitch LP) and a 64-vector
// in LDS, by all 256 threads: thread (row, quarter) sums 16 columns, the four
// quarters are added in fixed order.  Result to LDS out[] (if non-null) and to
// reg[0] of threads 0..63 (if non-null).  Ends with a barrier.
__device__ __forceinline__ void gemv64(const double *M, const double *v, double (*part)[NB],
                                       double *out, double scale, double *reg = nullptr)
{
    const int tid = threadIdx.x, row = tid & 63, qq = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int c = 16 * qq; c < 16 * qq + 16; c++) s = fma(M[row * LP + c], v[c], s);
    part[qq][row] = s;
    __syncthreads();
    if (tid < NB) {
        const double t = scale * (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
        if (out) out[tid] = t;
        if (reg) reg[0] = t;
    }
    __syncthreads();
}

// out[c] = scale * sum_r M[r][c] v[r] (M^T v), same thread split and order as gemv64
__device__ __forceinline__ void gemv64_t(const double *M, const double *v, double (*part)[NB],
                                         double *out, double scale)
{
    const int tid = threadIdx.x, c = tid & 63, qq = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int r = 16 * qq; r < 16 * qq + 16; r++) s = fma(M[r * LP + c], v[r], s);
    part[qq][c] = s;
    __syncthreads();
    if (tid < NB) out[tid] = scale * (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
    __syncthreads();
}

static __device__ __forceinline__ double rdlane(double v, int l)
{
    const long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffLL), l);
    const int hi = __builtin_amdgcn_readlane((int)(u >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// lane q's value to every lane of its 16-lane row (DPP row_newbcast, one
// v_mov_b64_dpp; no SGPR round trip).  q must fold to a constant.
template <int Q> __device__ __forceinline__ double rowbcast_c(double v)
{
    const long long u = __builtin_bit_cast(long long, v);
    const long long r = __builtin_amdgcn_mov_dpp(u, 0x150 + Q, 0xf, 0xf, true);
    return __builtin_bit_cast(double, r);
}

static __device__ __forceinline__ double rowbcast(double v, int q)
{
    switch (q) {
    case 0: return rowbcast_c<0>(v);
    case 1: return rowbcast_c<1>(v);
    case 2: return rowbcast_c<2>(v);
    case 3: return rowbcast_c<3>(v);
    case 4: return rowbcast_c<4>(v);
    case 5: return rowbcast_c<5>(v);
    case 6: return rowbcast_c<6>(v);
    case 7: return rowbcast_c<7>(v);
    case 8: return rowbcast_c<8>(v);
    case 9: return rowbcast_c<9>(v);
    case 10: return rowbcast_c<10>(v);
    case 11: return rowbcast_c<11>(v);
    case 12: return rowbcast_c<12>(v);
    case 13: return rowbcast_c<13>(v);
    case 14: return rowbcast_c<14>(v);
    default: return rowbcast_c<15>(v);
    }
}

// One wave: Cholesky of the 16x16 diagonal block at (o, o) of As and its
// inverse (lane r keeps row r of L and column r of L^-1 in registers; column
// broadcasts by DPP, pivots by readlane).  L (zero upper) -> As, L^-1 (zero
// upper) -> Bs.  The inverse's right-looking substitution (x_t /= L_tt,
// x_q -= L_qt x_t) runs inside the factor loop: its step t needs only column t
// of L, final at iteration t, and shares that column's DPP broadcasts L_qt with
// the rank-1 update -- its FMAs fill the latency of the next pivot's rsqrt
// chain instead of forming a second dependent loop (same operations in the
// same order as a separate loop: bit-identical).
__device__ __forceinline__ bool wave_factor16(double *As, double *Bs, int o)
{
    const int r = threadIdx.x & 63;
    double d[16], x[16];
#pragma unroll
    for (int c = 0; c < 16; c++) d[c] = (r < 16) ? As[(o + r) * LP + o + c] : 0.0;
#pragma unroll
    for (int q = 0; q < 16; q++) x[q] = (q == r) ? 1.0 : 0.0;
    // 1/sqrt of a pivot: hardware estimate + two Newton steps (full fp64).  No
    // test on the chain: a pivot <= 0 (or NaN) makes its diagonal entry
    // piv * rsq(piv) NaN, which the check after the loop finds
    auto rsq = [&](double piv) {
        double y = __builtin_amdgcn_rsq(piv);
        const double hp = 0.5 * piv;
        y = y * fma(-hp * y, y, 1.5);
        y = y * fma(-hp * y, y, 1.5);
        return y;
    };
    // pivots reach every lane of the row by a DPP broadcast (a VGPR: no
    // readlane -> SGPR -> VALU hazard wait on the chain)
    double y = rsq(rowbcast_c<0>(d[0]));
#pragma unroll
    for (int c = 0; c < 16; c++) {
        // Unpredicated: lane c's d[c] * y is its pivot times y, the diagonal
        // of L; lanes r < c scale / update only their upper part, which is
        // never broadcast (broadcasts read lanes q > c) and is zeroed at the
        // store below.
        d[c] = d[c] * y;
        x[c] = x[c] * y;
        // look-ahead: column c+1 first, so the next pivot's rsqrt chain can
        // overlap the rest of this column's rank-1 update
        if (c + 1 < 16) {
            const double b = rowbcast(d[c], c + 1);
            d[c + 1] = fma(-d[c], b, d[c + 1]);
            y = rsq(rowbcast(d[c + 1], c + 1));
            x[c + 1] = fma(-b, x[c], x[c + 1]);
        }
#pragma unroll
        for (int q = c + 2; q < 16; q++) {
            const double b = rowbcast(d[c], q);
            d[q] = fma(-d[c], b, d[q]);
            x[q] = fma(-b, x[c], x[q]);
        }
        // keep each column's inverse updates with its broadcasts: left alone,
        // the compiler sinks them below the loop and parks the 120 broadcasts
        // in AGPRs until then (an empty asm that "modifies" x pins them here)
#pragma unroll
        for (int q = c; q < 16; q++) asm volatile("" : "+v"(x[q]));
    }
    double dg = 1.0;   // lane r's diagonal entry L_rr = sqrt(pivot r)
#pragma unroll
    for (int c = 0; c < 16; c++)
        if (r == c) dg = d[c];
    const bool ok = __all(r >= 16 || (dg > 0.0 && dg < __builtin_inf()));
    if (r < 16) {
#pragma unroll
        for (int c = 0; c < 16; c++) As[(o + r) * LP + o + c] = (c <= r) ? d[c] : 0.0;
#pragma unroll
        for (int c = 0; c < 16; c++) Bs[(o + c) * LP + o + r] = x[c];
    }
    return ok;
}

// The 256-thread workgroup factors the 64x64 SPD tile in As (row-major, lower
// used) and inverts the factor, blocked by 16 (blocks 0..3).  Per block column
// k one wave factors the diagonal block (wave_factor16: L_kk and its inverse),
// the panel blocks L_ik = A_ik Dinv_kk^T follow on the matrix pipe, then the
// trailing blocks A_ij -= L_ik L_jk^T.  Look-ahead schedule: wave 0 updates
// the next diagonal block first and factors it at once, while the other waves
// finish the trailing blocks and form the off-diagonal blocks of L^-1,
//     Li_ij = -Li_ii sum_{t=j}^{i-1} L_it Li_tj,
// as soon as their inputs exist -- the critical path is the four diagonal
// factorisations plus three panel steps.  Every block is formed by exactly
// the operations of the plain right-looking order, so the result is the
// same bit for bit.  Writes L to the lower triangle of As (the upper
// triangle is zeroed only if zero_upper: the 16x16 blocks above the diagonal
// keep A otherwise) and L^-1 (zero upper) to Li.  Returns false on a
// non-positive pivot.  The caller synchronises after filling As; the result
// is visible after return.
__device__ __forceinline__ bool block_potrf_inv(double *As, double *Li, bool zero_upper = true)
{
    __shared__ double Xs[4][16 * LP];
    __shared__ __attribute__((aligned(16))) int bad;   // keeps the static LDS a
                                                       // multiple of 16 B (G17)
    const int tid = threadIdx.x, w = tid >> 6;
    // one trailing block (i, j) of block column k: A_ij -= L_ik L_jk^T
    auto trail = [&](int i, int j, int k) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nt(As, 16 * i, 16 * k, As, 16 * j, 16 * k, acc);
        put16(As, 16 * i, 16 * j, acc, -1.0, true);
    };
    // one panel block: L_ik = A_ik Dinv_kk^T
    auto panel = [&](int i, int k) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nt(As, 16 * i, 16 * k, Li, 16 * k, 16 * k, acc);
        put16(As, 16 * i, 16 * k, acc, 1.0, false);
    };
    // one off-diagonal block of the inverse, Li_ij (i > j), by wave w (> 0)
    auto inv = [&](int i, int j) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int t = j; t < i; t++) acc = mfma16_nn(As, 16 * i, 16 * t, Li, 16 * t, 16 * j, acc);
        put16(Xs[w], 0, 0, acc, 1.0, false);
        d4 acc2 = {0.0, 0.0, 0.0, 0.0};
        acc2 = mfma16_nn(Li, 16 * i, 16 * i, Xs[w], 0, 0, acc2);
        put16(Li, 16 * i, 16 * j, acc2, -1.0, false);
    };
    auto f16 = [&](int k) {
        if (!wave_factor16(As, Li, 16 * k) && (tid & 63) == 0) bad = 1;
    };
    // the six 16x16 blocks above the diagonal of L^-1 (everything else is
    // written below); ordered before their readers by the step barriers
    for (int q = tid; q < 6 * 256; q += blockDim.x) {
        const int b = q >> 8, e = q & 255;
        const int bi = b < 3 ? 0 : (b < 5 ? 1 : 2), bj = b < 3 ? b + 1 : (b < 5 ? b - 1 : 3);
        Li[(16 * bi + (e >> 4)) * LP + 16 * bj + (e & 15)] = 0.0;
    }
    if (tid == 0) bad = 0;   // same wave as the writer below: program order
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        // A(k): wave 0 updates diagonal block k by column k-1 and factors it;
        // waves 1-3 apply column k-1 to the other trailing blocks
        if (w == 0) {
            if (k > 0) trail(k, k, k - 1);
            f16(k);
        } else if (k > 0) {
            int p = 0;
            for (int j = k; j < 4; j++)
                for (int i = j; i < 4; i++) {
                    if (i == k && j == k) continue;
                    if (1 + p % 3 == w) trail(i, j, k - 1);
                    p++;
                }
        }
        __syncthreads();
        // B(k): three tasks for waves 1-3 -- the panels of column k, then the
        // inverse blocks of block row k
        if (w >= 1) {
            const int t = w - 1;
            if (t < 3 - k)
                panel(k + 1 + t, k);
            else
                inv(k, t - (3 - k));
        }
        __syncthreads();
    }
    if (zero_upper) {
        for (int q = tid; q < NB * NB; q += blockDim.x) {   // zero the upper triangle of L
            const int r = q >> 6, c = q & 63;
            if (c > r) As[r * LP + c] = 0.0;
        }
        __syncthreads();
    }
    return bad == 0;
}

// bounded spins of the in-launch hand-offs (then status[1]: re-solve without them)
#ifndef BA_BACK_SPIN_MAX
#define BA_BACK_SPIN_MAX 400000u
#endif

// ---------------------------------------------------------------------------
// Camera-aligned cyclic reduction on tiles of TB = NA * floor(32 / NA) rows
// (whole cameras; S rows g = TB * tile + r, r < TB, g < ld).  A tile lives in
// LDS as 32 x 32 (pitch LP, so the 16 x 16 MFMA helpers above apply): rows or
// columns r >= TB, or g >= ld, are padding -- zero, with a unit diagonal in a
// diagonal tile -- so the padded factorisation is that of the TB x TB tile
// bordered by an identity, and padding never leaks into real entries (the
// factors' padding rows / columns are zero off the diagonal).  Same algebra
// and launch structure as the 64-row kernels; the pivot chain per level is
// 32 columns instead of 64.
// ---------------------------------------------------------------------------
#define T32 32
static_assert(T32 == BA_TILE32, "the camera-aligned CR's tile height is the planner's");

// In-launch hand-offs of the one-launch cyclic reduction (k_cr32_fused):
// every byte one workgroup hands to another is stored write-through (sc1,
// 8-byte agent-scope atomic stores) and every load of it is an sc1 load
// (8-byte agent-scope atomic loads, L1 bypassed), one workgroup per CU, the
// flag an sc1 store after each storing wave's vmcnt(0) and a barrier: the
// first row of MI355X_MICROARCH.md's hand-off table (no acquire fence).
// SC = false: plain accesses (the per-level kernels, whose hand-offs cross a
// launch boundary).
template <bool SC = false>
__device__ __forceinline__ void load32(const double *__restrict__ S, long long lds, int TB,
                                       long long ld, int ti, int tj, double *T, bool transposed,
                                       bool diag)
{
    const int r = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const long long gr = (long long)TB * ti + r;
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = c0 + 8 * u;
        const long long gc = (long long)TB * tj + c;
        const bool ok = r < TB && c < TB && gr < ld && gc < ld;
        v[u] = ok ? ldg<SC>(S + gr + lds * gc) : ((diag && r == c) ? 1.0 : 0.0);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = c0 + 8 * u;
        if (transposed)
            T[c * LP + r] = v[u];
        else
            T[r * LP + c] = v[u];
    }
}

template <bool SC = false>
__device__ __forceinline__ void store32(double *__restrict__ S, long long lds, int TB,
                                        long long ld, int ti, int tj, const double *T)
{
    const int r = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const long long gr = (long long)TB * ti + r;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = c0 + 8 * u;
        const long long gc = (long long)TB * tj + c;
        if (r < TB && c < TB && gr < ld && gc < ld) stg<SC>(S + gr + lds * gc, T[r * LP + c]);
    }
}

// 32 x 32 LDS tile <-> row-major dst[r * 32 + c]
template <bool SC = false>
__device__ __forceinline__ void store_rm32(double *__restrict__ dst, const double *T)
{
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 4; u++) stg<SC>(dst + (r0 + 8 * u) * T32 + c, T[(r0 + 8 * u) * LP + c]);
}

template <bool SC = false>
__device__ __forceinline__ void load_rm32(const double *__restrict__ src, double *T)
{
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = ldg<SC>(src + (r0 + 8 * u) * T32 + c);
#pragma unroll
    for (int u = 0; u < 4; u++) T[(r0 + 8 * u) * LP + c] = v[u];
}

// One wave's copy of a whole 32 x 32 tile (load32 / load_rm32 with the 256
// threads' elements on the 64 lanes of one wave: the same values at the same
// LDS places), for the level records that wait for each operand's flag in the
// wave that loads it (cr32_level_body's PW form)
__device__ __forceinline__ void load32_wave(const double *__restrict__ S, long long lds, int TB,
                                            long long ld, int ti, int tj, double *T, bool transposed,
                                            bool diag)
{
    const int lane = threadIdx.x & 63, r = lane & 31, c0 = lane >> 5;
    const long long gr = (long long)TB * ti + r;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int c = c0 + 2 * u;
        const long long gc = (long long)TB * tj + c;
        const bool ok = r < TB && c < TB && gr < ld && gc < ld;
        v[u] = ok ? ldg<true>(S + gr + lds * gc) : ((diag && r == c) ? 1.0 : 0.0);
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int c = c0 + 2 * u;
        if (transposed)
            T[c * LP + r] = v[u];
        else
            T[r * LP + c] = v[u];
    }
}

__device__ __forceinline__ void load_rm32_wave(const double *__restrict__ src, double *T)
{
    const int lane = threadIdx.x & 63, c = lane & 31, r0 = lane >> 5;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = ldg<true>(src + (r0 + 2 * u) * T32 + c);
#pragma unroll
    for (int u = 0; u < 16; u++) T[(r0 + 2 * u) * LP + c] = v[u];
}

// acc (one 16 x 16 block per wave: rows 16 (w >> 1), cols 16 (w & 1)) of
// A B^T over K = 32 (nt form, as mfma_64x64)
__device__ __forceinline__ d4 mfma32_nt(const double *A, const double *Bt, d4 acc)
{
    const int w = threadIdx.x >> 6, ra = 16 * (w >> 1), cb = 16 * (w & 1);
    acc = mfma16_nt(A, ra, 0, Bt, cb, 0, acc);
    return mfma16_nt(A, ra, 16, Bt, cb, 16, acc);
}

__device__ __forceinline__ void put32(double *T, d4 acc, double scale, bool add)
{
    const int w = threadIdx.x >> 6;
    put16(T, 16 * (w >> 1), 16 * (w & 1), acc, scale, add);
}

// out[r] = scale * sum_c M[r][c] v[c] (t = 0) or sum_c M[c][r] v[c] (t = 1),
// r < 32: thread (r, part of 4 columns), the 8 parts added in fixed order
__device__ __forceinline__ void gemv32(const double *M, const double *v, double (*part)[T32],
                                       double *out, bool t)
{
    const int tid = threadIdx.x, r = tid & 31, pq = tid >> 5;
    double acc = 0.0;
#pragma unroll
    for (int c = 4 * pq; c < 4 * pq + 4; c++)
        acc = fma(t ? M[c * LP + r] : M[r * LP + c], v[c], acc);
    part[pq][r] = acc;
    __syncthreads();
    if (tid < T32)
        out[tid] = ((((((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) +
                     part[4][tid]) + part[5][tid]) + part[6][tid]) + part[7][tid];
    __syncthreads();
}

// One wave: wave_factor16's Cholesky of the 16x16 diagonal block at (o, o)
// of As, and forward substitutions z = L^-1 v of up to 48 more vectors in
// the same loop.  Every 16-lane row of the wave holds a copy of the factor
// rows (lane l: row l & 15), so each row's DPP broadcasts see the factor's
// column and the copies stay bit-identical; lanes 0..15 carry the identity
// (column r of L^-1 -> Li, if Li), lanes 16 + i (i < 16) vector i of segment
// lo and lanes 32 + i (i < 32) vector i of segment hi (in == nullptr: none).
// The substitutions ride on the factor's broadcasts, so a panel A L^-T (rows
// of A as the vectors) costs no separate stage.  Every lane issues the same
// 16 unconditional LDS loads for its start vector (e_r and zeros from a
// small LDS row), so the loads are in flight together and need no selects.  Lanes 0..15 write L (zero upper) to As.
// Returns false on a non-positive pivot.
struct vseg {
    const double *in;   // entry c of vector i: in[i * irs + c * ics]
    double *out;        // result entry c:      out[i * ors + c * ocs]
    int irs, ics, ors, ocs;
    int n;              // vectors (lanes 16 / 32 + i, i < n)
};

__device__ __forceinline__ bool wave_factor16x(double *As, double *Li, int o, vseg lo, vseg hi)
{
    // e_r for lanes r < 16 and zeros for idle lanes come from one LDS row
    // (ident[16] = 1), so every lane's start vector is one strided read
    __shared__ double ident[33];
    const int lane = threadIdx.x & 63, r = lane & 15;
    if (lane < 33) ident[lane] = lane == 16 ? 1.0 : 0.0;
    const bool up = lane >= 32;
    const int idx = up ? lane - 32 : lane - 16;
    const double *sin = up ? hi.in : lo.in;
    const bool act = lane >= 16 && sin != nullptr && idx < (up ? hi.n : lo.n);
    const double *pin =
        act ? sin + idx * (up ? hi.irs : lo.irs) : (lane < 16 ? ident + 16 - r : ident);
    const int ics = act ? (up ? hi.ics : lo.ics) : 1;
    double d[16], x[16];
#pragma unroll
    for (int c = 0; c < 16; c++) d[c] = As[(o + r) * LP + o + c];
    __builtin_amdgcn_wave_barrier();   // ident written (same wave: LDS in order)
#pragma unroll
    for (int q = 0; q < 16; q++) x[q] = pin[q * ics];
    auto rsq = [&](double piv) {
        double y = __builtin_amdgcn_rsq(piv);
        const double hp = 0.5 * piv;
        y = y * fma(-hp * y, y, 1.5);
        y = y * fma(-hp * y, y, 1.5);
        return y;
    };
    double y = rsq(rowbcast_c<0>(d[0]));
#pragma unroll
    for (int c = 0; c < 16; c++) {
        d[c] = d[c] * y;
        x[c] = x[c] * y;
        if (c + 1 < 16) {
            const double b = rowbcast(d[c], c + 1);
            d[c + 1] = fma(-d[c], b, d[c + 1]);
            y = rsq(rowbcast(d[c + 1], c + 1));
            x[c + 1] = fma(-b, x[c], x[c + 1]);
        }
#pragma unroll
        for (int q = c + 2; q < 16; q++) {
            const double b = rowbcast(d[c], q);
            d[q] = fma(-d[c], b, d[q]);
            x[q] = fma(-b, x[c], x[q]);
        }
#pragma unroll
        for (int q = c; q < 16; q++) asm volatile("" : "+v"(x[q]));
    }
    double dg = 1.0;
#pragma unroll
    for (int c = 0; c < 16; c++)
        if (r == c) dg = d[c];
    const bool ok = __all(lane >= 16 || (dg > 0.0 && dg < __builtin_inf()));
    if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; c++) As[(o + r) * LP + o + c] = (c <= r) ? d[c] : 0.0;
        if (Li) {
#pragma unroll
            for (int c = 0; c < 16; c++) Li[(o + c) * LP + o + r] = x[c];
        }
    } else if (act) {
        double *po = (up ? hi.out : lo.out) + idx * (up ? hi.ors : lo.ors);
        const int ocs = up ? hi.ocs : lo.ocs;
#pragma unroll
        for (int c = 0; c < 16; c++) po[c * ocs] = x[c];
    }
    return ok;
}

// The 32 x 32 Cholesky of As (lower; block (0, 1) keeps A) and, if Li, L^-1
// (row-major, zero upper) -> Li, and, if Cm, the panel Cm L^-T in place (32
// rows), as two wave_factor16x stages with one MFMA stage between them:
//   F0 (wave 0): L00; L10 = A10 L00^-T (lanes 16..31, in place); P0 = C0
//      L00^-T (lanes 32..63, in place) -- or, without a panel and with rv,
//      y0 = L00^-1 r0 (lane 32) -> yv; Li00 (lanes 0..15).  Waves 1..3 run
//      side(w) meanwhile (work F1 needs but F0 does not, e.g. the rest of a
//      pending update of A11 or C1).
//   M: A11 -= L10 L10^T (wave 0); C1 -= P0 L10^T (waves 1, 2) or r1 -= L10
//      y0 (wave 1, in rv); V = -L10 Li00 (wave 3, for Li10).
//   F1 (wave 0): L11; P1 = C1 L11^-T (lanes 32..63) or y1 = L11^-1 r1
//      (lane 32); Li11 (lanes 0..15); Li10 = L11^-1 V (lanes 16..31).
// The critical path is the two 16-pivot chains plus one MFMA stage: the
// panel and the inverse's off-diagonal block need no stage of their own.
// The caller synchronises after filling As / Cm; results visible on return.
// CH_ST(k): the diagnostic build's stamps of the two stages (ba_chol.hip
// defines it before this header; nothing elsewhere)
#ifndef CH_ST
#define CH_ST(k)
#endif

template <class Side>
__device__ __forceinline__ bool cr32_chol(double *As, double *Li, double *Cm, double *Xs,
                                          double *rv, double *yv, Side side)
{
    __shared__ int bad32;
    const int tid = threadIdx.x, w = tid >> 6;
    if (Li) Li[(tid >> 4) * LP + 16 + (tid & 15)] = 0.0;   // block (0, 1) of L^-1
    if (w == 0) {
        const vseg lo{As + 16 * LP, As + 16 * LP, LP, 1, LP, 1, 16};   // A10 rows -> L10
        const vseg hi = Cm ? vseg{Cm, Cm, LP, 1, LP, 1, 32}            // C0 rows -> P0
                           : vseg{rv, yv, 0, 1, 0, 1, 1};              // or r0 -> y0
        const bool ok = wave_factor16x(As, Li, 0, lo, hi);
        if (tid == 0) bad32 = ok ? 0 : 1;
    } else {
        side(w);
    }
    __syncthreads();
    CH_ST(0);
    if (w == 0) {   // A11 -= L10 L10^T
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nt(As, 16, 0, As, 16, 0, acc);
        put16(As, 16, 16, acc, -1.0, true);
    } else if (w <= 2) {   // C1 -= P0 L10^T, rows 16 (w - 1) ..
        if (Cm) {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            acc = mfma16_nt(Cm, 16 * (w - 1), 0, As, 16, 0, acc);
            put16(Cm, 16 * (w - 1), 16, acc, -1.0, true);
        } else if (rv && w == 1 && (tid & 63) < 16) {   // r1' = r1 - L10 y0
            const int r = tid & 63;
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < 16; c++) t = fma(As[(16 + r) * LP + c], yv[c], t);
            rv[16 + r] = rv[16 + r] - t;
        }
    } else if (Li) {   // V = -L10 Li00
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nn(As, 16, 0, Li, 0, 0, acc);
        put16(Xs, 0, 0, acc, -1.0, false);
    }
    __syncthreads();
    CH_ST(1);
    if (w == 0) {
        // V's columns -> Li10's columns; C1 rows -> P1, or r1' -> y1
        const vseg lo{Li ? Xs : nullptr, Li ? Li + 16 * LP : nullptr, 1, LP, 1, LP, 16};
        const vseg hi = Cm ? vseg{Cm + 16, Cm + 16, LP, 1, LP, 1, 32}
                           : vseg{rv ? rv + 16 : nullptr, yv ? yv + 16 : nullptr, 0, 1, 0, 1, 1};
        const bool ok = wave_factor16x(As, Li, 16, lo, hi);
        if (tid == 0 && !ok) bad32 = 1;
    }
    __syncthreads();
    return bad32 == 0;
}

// The envelope's 64 x 64 diagonal factor and L^-1 (row-major, zero upper, in
// Bs) as two cr32_chol factors: F(A00) -> L00, Li00 and the panel L10 = A10
// L00^-T on the same pivot chains; then A11 -= L10 L10^T (waves 0-2, its
// three lower 16-blocks) beside T = L10 Li00 (into Bs's block (1, 0)); F(A11)
// -> L11, Li11; Li10 = -Li11 T.  Two 32-row factors (~8.2k cycles each,
// profiles/r04c_ubench_cr32.txt) instead of four dependent 16-row stages with
// their updates in between (block_potrf_inv, ~29.5k cycles).  Xs: 16 x LP
// scratch.  Ends with a barrier.
__device__ __forceinline__ bool potrf64_via32(double *As, double *Bs, double *Xs)
{
    const int tid = threadIdx.x, w = tid >> 6;
    for (int q = tid; q < 32 * 32; q += blockDim.x) Bs[(q >> 5) * LP + 32 + (q & 31)] = 0.0;
    bool ok = cr32_chol(As, Bs, As + 32 * LP, Xs, nullptr, nullptr, [](int) {});
    {
        // A11 -= L10 L10^T: blocks (32, 32), (48, 32), (48, 48) by waves 0..2;
        // T = L10 Li00 blocks (32 + 16 (u >> 1), 16 (u & 1)), u = w and w + 4 - 1 ...
        const int ri = w == 0 ? 32 : 48, ci = w == 2 ? 48 : 32;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (w < 3) {
            acc = mfma16_nt(As, ri, 0, As, ci, 0, acc);
            acc = mfma16_nt(As, ri, 16, As, ci, 16, acc);
        }
        // T blocks: wave 3 takes (32, 0) and (32, 16), waves 0 / 1 take (48, 0) / (48, 16)
        d4 t0 = {0.0, 0.0, 0.0, 0.0}, t1 = {0.0, 0.0, 0.0, 0.0};
        if (w == 3) {
            t0 = mfma16_nn(As, 32, 0, Bs, 0, 0, t0);
            t0 = mfma16_nn(As, 32, 16, Bs, 16, 0, t0);
            t1 = mfma16_nn(As, 32, 16, Bs, 16, 16, t1);   // Li00 block (0, 1) is zero
        } else if (w < 2) {
            t0 = mfma16_nn(As, 48, 0, Bs, 0, 16 * w, t0);
            t0 = mfma16_nn(As, 48, 16, Bs, 16, 16 * w, t0);
        }
        if (w < 3) put16(As, ri, ci, acc, -1.0, true);
        if (w == 3) {
            put16(Bs, 32, 0, t0, 1.0, false);
            put16(Bs, 32, 16, t1, 1.0, false);
        } else if (w < 2) {
            put16(Bs, 48, 16 * w, t0, 1.0, false);
        }
    }
    __syncthreads();
    ok = cr32_chol(As + 32 * LP + 32, Bs + 32 * LP + 32, nullptr, Xs, nullptr, nullptr,
                   [](int) {}) && ok;
    {   // Li10 = -Li11 T, block (32 + 16 (w >> 1), 16 (w & 1)) by wave w
        const int ri = 32 + 16 * (w >> 1), cj = 16 * (w & 1);
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nn(Bs, ri, 32, Bs, 32, cj, acc);
        acc = mfma16_nn(Bs, ri, 48, Bs, 48, cj, acc);
        __syncthreads();
        put16(Bs, ri, cj, acc, -1.0, false);
    }
    __syncthreads();
    return ok;
}
