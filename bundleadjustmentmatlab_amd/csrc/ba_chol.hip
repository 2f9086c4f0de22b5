// ba_chol.hip -- dense reduced-camera solve on gfx950: blocked right-looking
// tile Cholesky with fp64 MFMA (v_mfma_f64_16x16x4_f64) + triangular solves.
//
// Replaces da = pinv(S) * e_ (toolbox/bundle/bundle_euclid.m:193).  S is
// symmetric positive definite once its exactly-zero rows (fixed parameters,
// App. A Q2/Q8) are given a unit diagonal (k_assemble_tiles), and on that matrix
// pinv and the Cholesky solve agree to conditioning-limited rounding.  A
// non-positive pivot sets status[0]; the host then takes da = pinv(S) e_
// (rocSOLVER dsyevd, ba_solver.cpp pinv_fallback), as bundle_euclid.m:193 does.
//
// Storage: S column major, leading dimension lds (multiple of NB = 64), lower
// triangle.  Tile envelope: tile row i of S (hence of L: the profile is
// preserved by Cholesky) is zero left of tile column tfirst[i]; every kernel
// below visits only tiles inside the envelope, which is exact (the skipped
// tiles are zero and stay zero).  dense_solve = 1 visits every lower tile.
//
// Per tile column k (one launch, k_factor_step):
//   WG 0     : applies column k-1's update to A_kk, factors L_kk, forms
//              L_kk^-1 and y_k = L_kk^-1 r_k (forward solve folded in);
//   WG b > 0 : applies column k-1's update to A_ik, redoes A_kk's update and
//              factorisation in LDS and forms the panel tile L_ik = A_ik L_kk^-T
//              (MFMA), r_i -= L_ik y_k;
//   the rest : column k-1's trailing update A_ij -= L_i,k-1 L_j,k-1^T of the
//              envelope pairs below row k (MFMA)
// then the backward solve x_k = L_kk^-T z_k, z_j -= L_kj^T x_k (one launch,
// k_backward_all, or per column k_backward).
//
// Solvers on top of the tiles (chol_plan_build, ba_chol_plan.cpp, picks one): block cyclic
// reduction when S is tile-tridiagonal (k_cr32_fused on camera-aligned 30-row
// tiles); else the envelope Cholesky, on a nested-dissection camera order
// (arcs side by side in k_factor_multi, separator SYRK k_sep_update /
// k_sep_reduce, then the separator) when that shortens the chain of columns;
// the sequential k_chol_seq in parity mode.
#include "ba_internal.h"
#include "ba_camera.h"
#include "ba_chol.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <cstdio>
#include <utility>
#include <climits>
#include <cstdlib>
#include <vector>

#ifdef BA_STAMPS
// diagnostic build: cr32_chol's two stages per workgroup (ba_chol_tile.h;
// tools/cr_timeline.py)
__device__ unsigned long long g_chst[8192][2];
#define CH_ST(k)                                                                          \
    do {                                                                                  \
        if (threadIdx.x == 0 && blockIdx.x < 8192)                                        \
            g_chst[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();                     \
    } while (0)
extern "C" int vlgba_debug_chstamps(unsigned long long *out, int nrec)
{
    if (nrec > 8192) nrec = 8192;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chst), sizeof(unsigned long long) * 2 * nrec) ==
                   hipSuccess
               ? 0
               : -1;
}
#endif
#include "ba_chol_tile.h"

// ---------------------------------------------------------------------------
// One tile column k of the envelope Cholesky, with the trailing update of
// column k-1 folded in (one launch per column instead of two):
//   blockIdx 0        : A_kk -= L_{k,k-1} L_{k,k-1}^T (if column k-1 reaches
//                       row k), factor it, L_kk^-1, y_k = L_kk^-1 r_k
//   1 .. T            : panel tile i = pan[b-1]: A_ik -= L_{i,k-1} L_{k,k-1}^T,
//                       the same update + factorisation of A_kk in LDS
//                       (bit-identical), L_ik = A_ik L_kk^-T, r_i -= L_ik y_k
//   T+1 ..            : the rest of column k-1's trailing update,
//                       A_ij -= L_{i,k-1} L_{j,k-1}^T for envelope pairs of
//                       column k-1 with k < j <= i
// Every tile receives the same operations in the same order as the two-launch
// schedule (acc formed from zero, then A + (-1) acc): bit-identical results.
// pan / prev: the envelope rows below k / below k-1 (ascending), T / Tp their
// counts (Tp = 0 for k = 0).
// ---------------------------------------------------------------------------
#ifdef BA_STAMPS
// per tile column k: [0..3] workgroup 0 entry / factor start / factor end /
// exit, [4..7] the same for workgroup 1 (first panel tile), [8] the last exit
#define FS_MAX 4096
__device__ unsigned long long g_fst[FS_MAX][9];
extern "C" int vlgba_debug_fstamps(unsigned long long *out, int n)
{
    if (n > FS_MAX) n = FS_MAX;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fst), sizeof(unsigned long long) * 9 * n) ==
                   hipSuccess
               ? 0
               : -1;
}
#define FS_ST(q)                                                                          \
    do {                                                                                  \
        if (threadIdx.x == 0 && b <= 1 && k < FS_MAX)                                     \
            g_fst[k][4 * b + (q)] = __builtin_amdgcn_s_memrealtime();                     \
    } while (0)
#define FS_END()                                                                          \
    do {                                                                                  \
        if (threadIdx.x == 0 && k < FS_MAX)                                               \
            atomicMax(&g_fst[k][8], (unsigned long long)__builtin_amdgcn_s_memrealtime()); \
    } while (0)
#else
#define FS_ST(q)
#define FS_END()
#endif

// sep0: the nested dissection's first separator row tile (INT_MAX: none):
// an arc column leaves the separator's rhs to k_sep_update (two arcs'
// columns run in the same launch) and its separator x separator trailing
// pairs, which the host does not launch (they end each pair enumeration).
// kflag (one-launch hand-off, may be null): workgroup 0 publishes L_kk^-1 and
// y_k (write-through stores, then flag k = epoch) and the panel workgroups
// take them from there instead of updating and factoring A_kk themselves --
// the same bits (workgroup 0's factor is the one they would recompute), with
// the panel's own pending update overlapping workgroup 0's factor.  A panel
// workgroup only waits on workgroup 0 of its column, which has a lower index
// (dispatched first); a spin that gives up sets status[1] and the host
// re-solves with kflag = null.
__device__ __forceinline__ void factor_step_body(double *__restrict__ S, long long lds, int k,
                                                 const int *__restrict__ pan, int T,
                                                 const int *__restrict__ prev, int Tp,
                                                 double *__restrict__ linv,
                                                 double *__restrict__ rhs,
                                                 double *__restrict__ y,
                                                 double *__restrict__ status, int b, int sep0,
                                                 unsigned *__restrict__ kflag, unsigned epoch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP, *Cs = sm + 2 * NB * LP;
    __shared__ double yk[NB], rk[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x;
    const bool kin = Tp > 0 && prev[0] == k;   // column k-1 reaches row k
    d4 acc[2][2];
    FS_ST(0);
    if (b > T) {
        // trailing pairs of column k-1 below row k (k_syrk's enumeration over
        // prev without k)
        const int *pl = prev + (kin ? 1 : 0);
        const int Tr = Tp - (kin ? 1 : 0);
        int q = b - T - 1, jj = 0;
        while (q >= Tr - jj) {
            q -= Tr - jj;
            jj++;
        }
        const int j = pl[jj], i = pl[jj + q];
        double va[16], vb[16], vc[16];
        fetch_tile(S, lds, i, k - 1, va);
        fetch_tile(S, lds, j, k - 1, vb);
        fetch_tile(S, lds, i, j, vc);
        put_tile(As, va, false);
        put_tile(Bs, vb, false);
        put_tile(Cs, vc, false);
        __syncthreads();
        mfma_64x64(As, Bs, acc);
        acc_to_lds(acc, Cs, -1.0, true);
        __syncthreads();
        store_tile(S, lds, i, j, Cs);
        FS_END();
        return;
    }
    const int i = b > 0 ? pan[b - 1] : k;
    const bool hand = kflag != nullptr && b > 0;   // a panel taking L_kk^-1 / y_k from workgroup 0
    // every tile this workgroup reads, fetched at once (one memory latency
    // instead of three dependent ones): A_ik, L_k,k-1, A_kk, L_i,k-1
    double vc[16], va[16], vb[16], vk[16];
    if (b > 0) fetch_tile(S, lds, i, k, vc);
    if (kin) fetch_tile(S, lds, k, k - 1, vb);
    if (!hand) fetch_tile(S, lds, k, k, vk);
    bool iin = false;   // column k-1 reaches row i (panel tiles only): a wave-wide search
    if (b > 0 && kin) {
        const int lane = tid & 63;
        for (int t0 = 1; t0 < Tp && !iin; t0 += 64)
            iin = __any(t0 + lane < Tp && prev[t0 + lane] == i);
    }
    if (iin) fetch_tile(S, lds, i, k - 1, va);
    if (!hand && tid < NB) rk[tid] = rhs[(long long)NB * k + tid];
    if (b > 0) put_tile(Cs, vc, false);
    if (iin) put_tile(As, va, false);
    if (kin) put_tile(Bs, vb, false);
    __syncthreads();
    if (iin) {   // A_ik's pending update of column k-1
        mfma_64x64(As, Bs, acc);
        __syncthreads();
        acc_to_lds(acc, Cs, -1.0, true);
    }
    if (hand) {
        if (tid < 64) {   // wave 0 waits for workgroup 0's flag
            for (unsigned spins = 0;; spins++) {
                const unsigned f = __hip_atomic_load((const gu32_t *)(kflag + k), __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                if (f == epoch) break;
                if (spins >= BA_BACK_SPIN_MAX) {
                    if (tid == 0) status[1] = 1.0;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        __syncthreads();
        {   // L_kk^-1 (row-major, write-through) -> Bs, y_k -> yk (agent-scope loads)
            const double *lo = linv + (long long)NB * NB * k;
            const int c = tid & 63, r0 = tid >> 6;
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = ldg<true>(lo + (r0 + 4 * u) * NB + c);
#pragma unroll
            for (int u = 0; u < 16; u++) Bs[(r0 + 4 * u) * LP + c] = v[u];
            if (tid < NB) yk[tid] = ldg<true>(y + (long long)NB * k + tid);
        }
        __syncthreads();
        FS_ST(1);
        FS_ST(2);
    } else {
    // A_kk and its pending update
    if (kin) mfma_64x64(Bs, Bs, acc);
    __syncthreads();
    put_tile(As, vk, false);
    __syncthreads();
    if (kin) {
        acc_to_lds(acc, As, -1.0, true);
        __syncthreads();
    }
    FS_ST(1);
    const bool ok = potrf64_via32(As, Bs, As + 32);   // scratch: A's upper-right block
    FS_ST(2);
    gemv64(Bs, rk, part, yk, 1.0);            // y_k = L^-1 r_k
    if (b == 0 && kflag) {   // published for the column's panel workgroups
        double *lo = linv + (long long)NB * NB * k;
        for (int q = tid; q < NB * NB; q += blockDim.x)
            stg<true>(lo + q, Bs[(q >> 6) * LP + (q & 63)]);
        if (tid < NB) stg<true>(y + (long long)NB * k + tid, yk[tid]);
        if (tid == 0 && !ok) status[0] = 1.0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
        __syncthreads();
        if (tid == 0)
            __hip_atomic_store((gu32_t *)(kflag + k), epoch, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        FS_ST(3);
        FS_END();
        return;
    }
    if (b == 0) {
        // L_kk is NOT stored back to S(k, k): the panel workgroups of this
        // launch read A_kk from there, and one that starts after this store
        // (a busy GPU: not every workgroup is resident at once) would factor
        // L_kk instead of A_kk.  Nothing reads L_kk later (the backward solve
        // takes L_kk^-1 from linv, the next columns only off-diagonal tiles).
        double *lo = linv + (long long)NB * NB * k;
        for (int q = tid; q < NB * NB; q += blockDim.x) lo[q] = Bs[(q >> 6) * LP + (q & 63)];
        if (tid < NB) y[(long long)NB * k + tid] = yk[tid];
        if (tid == 0 && !ok) status[0] = 1.0;
        FS_ST(3);
        FS_END();
        return;
    }
    }   // (!hand)
    mfma_64x64(Cs, Bs, acc);   // L_ik[r][c] = sum_t A_ik[r][t] Li[c][t]
    __syncthreads();
    acc_to_lds(acc, Cs, 1.0, false);
    __syncthreads();
    store_tile(S, lds, i, k, Cs);
    double ri[1];
    gemv64(Cs, yk, part, nullptr, 1.0, ri);   // (L_ik y_k)[tid] for tid < 64
    if (tid < NB && i < sep0) rhs[(long long)NB * i + tid] -= ri[0];
    FS_ST(3);
    FS_END();
}

// Runner mode (k_env_runner beside the column launches; the default,
// VLGBA_ENV_RUNNER=0 turns it off): a
// persistent workgroup per run of columns [k0, kend) factors every diagonal
// tile and forms the first panel tile L_k+1,k itself, so the column launches
// lose workgroup 0 and that panel.  The tiles the two exchange inside a launch
// go through sc1 stores / loads and a flag each (epoch = fac_epoch):
//   lflag[k]   L_k,k-1 stored by the runner (the panels' pending update reads it)
//   dflag[k]   A_kk's last trailing update (column k-2) stored
//   uflag[k+1] A_k+1,k's pending update of column k-1 stored (the runner's panel)
//   pflag[k+1] r_k+1's update by column k-1's panel stored (before the runner's)
// (a profile: column c reaches row i for every c from row i's first column on,
// so these are the only writes the runner waits for; every other write it
// reads was made by a launch that ended before one of those flags was set).
struct env_rm {
    unsigned *lflag, *dflag, *uflag, *pflag;
    unsigned *rto;   // a runner hand-off gave up (the host turns this context's runner off)
    int kend;   // the run's end column (exclusive); 0: not in runner mode
};

// wave 0 spins on flag[idx] == epoch (bounded; timeout: status[1] and the
// runner's own word *rto); all waves then pass a barrier.  Returns false on a
// timeout.
__device__ __forceinline__ bool env_wait(const unsigned *flag, int idx, unsigned epoch,
                                         double *status, unsigned *rto)
{
    __shared__ int to;
    const int tid = threadIdx.x;
    if (tid < 64) {
        bool ok = false;
        for (unsigned spins = 0; spins < BA_BACK_SPIN_MAX; spins++) {
            const unsigned f = __hip_atomic_load((const gu32_t *)(flag + idx), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            if (f == epoch) {
                ok = true;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (tid == 0) {
            to = ok ? 0 : 1;
            if (!ok) {
                status[1] = 1.0;
                __hip_atomic_store((gu32_t *)rto, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    __syncthreads();
    return to == 0;
}

__device__ __forceinline__ void env_publish(unsigned *flag, int idx, unsigned epoch)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store((gu32_t *)(flag + idx), epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// factor_step_body with the in-launch hand-off on two LDS tiles instead of
// three (two workgroups per CU): the pending updates' operands come straight
// from S (mfma_64x64_glb), workgroup 0 factors in As -> Bs, a panel keeps
// A_ik in As and L_kk^-1 in Bs, a trailing pair its C tile in As.  The same
// operations in the same order: bit-identical to factor_step_body.
__device__ __forceinline__ void factor_step_two(double *__restrict__ S, long long lds, int k,
                                                const int *__restrict__ pan, int T,
                                                const int *__restrict__ prev, int Tp,
                                                double *__restrict__ linv,
                                                double *__restrict__ rhs,
                                                double *__restrict__ y,
                                                double *__restrict__ status, int b, int sep0,
                                                unsigned *__restrict__ kflag, unsigned epoch,
                                                int ntr, int tstride, env_rm R = env_rm{})
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP;
    __shared__ double yk[NB], rk[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x;
    const bool kin = Tp > 0 && prev[0] == k;   // column k-1 reaches row k
    d4 acc[2][2];
    FS_ST(0);
    if (b > T) {
        // trailing pairs q = b - T - 1 + u tstride (< ntr) of column k-1
        // below row k, one after another: fewer workgroups than pairs keeps
        // them off most CUs, so the diagonal factor's chain seldom shares one
        const int *pl = prev + (kin ? 1 : 0);
        const int Tr = Tp - (kin ? 1 : 0);
        for (int q0 = b - T - 1; q0 < ntr; q0 += tstride) {
            int q = q0, jj = 0;
            while (q >= Tr - jj) {
                q -= Tr - jj;
                jj++;
            }
            const int j = pl[jj], i = pl[jj + q];
            double vc[16];
            fetch_tile(S, lds, i, j, vc);
            mfma_64x64_glb(S, lds, i, j, k - 1, acc);
            put_tile(As, vc, false);
            __syncthreads();
            acc_to_lds(acc, As, -1.0, true);
            __syncthreads();
            if (R.kend && i == k + 1 && j == k + 1 && k + 1 < R.kend) {
                // A_k+1,k+1's last trailing update: the runner reads it at column k+1
                store_tile_sc(S, lds, i, j, As);
                env_publish(R.dflag, k + 1, epoch);
            } else {
                store_tile(S, lds, i, j, As);
            }
            __syncthreads();   // As read by every thread before the next pair's put
        }
        FS_END();
        return;
    }
    if (b == 0 && R.kend) {   // the runner factors A_kk
        FS_END();
        return;
    }
    if (b == 0) {   // A_kk's pending update, factor, L_kk^-1, y_k; published
        double vk[16];
        fetch_tile(S, lds, k, k, vk);
        if (tid < NB) rk[tid] = rhs[(long long)NB * k + tid];
        if (kin) mfma_64x64_glb(S, lds, k, k, k - 1, acc);
        put_tile(As, vk, false);
        __syncthreads();
        if (kin) {
            acc_to_lds(acc, As, -1.0, true);
            __syncthreads();
        }
        FS_ST(1);
        const bool ok = potrf64_via32(As, Bs, As + 32);
        FS_ST(2);
        gemv64(Bs, rk, part, yk, 1.0);   // y_k = L^-1 r_k
        double *lo = linv + (long long)NB * NB * k;
        for (int q = tid; q < NB * NB; q += blockDim.x)
            stg<true>(lo + q, Bs[(q >> 6) * LP + (q & 63)]);
        if (tid < NB) stg<true>(y + (long long)NB * k + tid, yk[tid]);
        if (tid == 0 && !ok) status[0] = 1.0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
        __syncthreads();
        if (tid == 0)
            __hip_atomic_store((gu32_t *)(kflag + k), epoch, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        FS_ST(3);
        FS_END();
        return;
    }
    // a panel tile: A_ik and its pending update, then L_ik = A_ik L_kk^-T
    const int i = pan[b - 1];
    double vc[16];
    fetch_tile(S, lds, i, k, vc);
    bool iin = false;   // column k-1 reaches row i: a wave-wide search
    if (kin) {
        const int lane = tid & 63;
        for (int t0 = 1; t0 < Tp && !iin; t0 += 64)
            iin = __any(t0 + lane < Tp && prev[t0 + lane] == i);
    }
    const bool lrun = R.kend && i == k + 1 && k + 1 < R.kend;   // the runner's panel
    if (lrun && !iin) {   // no pending update: the runner reads A_k+1,k as it is
        FS_END();
        return;
    }
    if (iin && R.kend) {   // L_k,k-1 is the runner's
        if (!env_wait(R.lflag, k, epoch, status, R.rto)) return;
        mfma_64x64_glb<true>(S, lds, i, k, k - 1, acc);
    } else if (iin) {
        mfma_64x64_glb(S, lds, i, k, k - 1, acc);
    }
    put_tile(As, vc, false);
    __syncthreads();
    if (iin) acc_to_lds(acc, As, -1.0, true);
    if (lrun) {   // A_k+1,k after its pending update, for the runner
        __syncthreads();
        store_tile_sc(S, lds, i, k, As);
        env_publish(R.uflag, k + 1, epoch);
        FS_END();
        return;
    }
    if (tid < 64) {   // wave 0 waits for workgroup 0's flag
        for (unsigned spins = 0;; spins++) {
            const unsigned f = __hip_atomic_load((const gu32_t *)(kflag + k), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            if (f == epoch) break;
            if (spins >= BA_BACK_SPIN_MAX) {
                if (tid == 0) status[1] = 1.0;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
    {   // L_kk^-1 (row-major, write-through) -> Bs, y_k -> yk (agent-scope loads)
        const double *lo = linv + (long long)NB * NB * k;
        const int c = tid & 63, r0 = tid >> 6;
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = ldg<true>(lo + (r0 + 4 * u) * NB + c);
#pragma unroll
        for (int u = 0; u < 16; u++) Bs[(r0 + 4 * u) * LP + c] = v[u];
        if (tid < NB) yk[tid] = ldg<true>(y + (long long)NB * k + tid);
    }
    __syncthreads();
    FS_ST(1);
    FS_ST(2);
    mfma_64x64(As, Bs, acc);   // L_ik[r][c] = sum_t A_ik[r][t] Li[c][t]
    __syncthreads();
    acc_to_lds(acc, As, 1.0, false);
    __syncthreads();
    store_tile(S, lds, i, k, As);
    double ri[1];
    gemv64(As, yk, part, nullptr, 1.0, ri);   // (L_ik y_k)[tid] for tid < 64
    if (R.kend && i == k + 2 && k + 2 < R.kend) {   // the runner updates r_k+2 next
        if (tid < NB) {
            double *rp = rhs + (long long)NB * i + tid;
            stg<true>(rp, ldg<true>(rp) - ri[0]);
        }
        env_publish(R.pflag, k + 2, epoch);
    } else if (tid < NB && i < sep0) {
        rhs[(long long)NB * i + tid] -= ri[0];
    }
    FS_ST(3);
    FS_END();
}

__global__ __launch_bounds__(256) void k_factor_step(double *__restrict__ S, long long lds, int k,
                                                     const int *__restrict__ pan, int T,
                                                     const int *__restrict__ prev, int Tp,
                                                     double *__restrict__ linv,
                                                     double *__restrict__ rhs,
                                                     double *__restrict__ y,
                                                     double *__restrict__ status,
                                                     unsigned *__restrict__ kflag, unsigned epoch,
                                                     int ntr, int tstride, env_rm R)
{
    if (kflag)
        factor_step_two(S, lds, k, pan, T, prev, Tp, linv, rhs, y, status, blockIdx.x, INT_MAX,
                        kflag, epoch, ntr, tstride, R);
    else
        factor_step_body(S, lds, k, pan, T, prev, Tp, linv, rhs, y, status, blockIdx.x, INT_MAX,
                         nullptr, 0);
}

// one step of every arc of the nested dissection: column k[t] of arc t takes
// workgroups [b0[t], b0[t+1]) (k_factor_step's roles), pan / prev as offsets
// into the panel list (nd_step, ba_chol_plan.h: grouped by role, or arc-major)
__global__ __launch_bounds__(256) void k_factor_multi(double *__restrict__ S, long long lds,
                                                      const int *__restrict__ pan_list,
                                                      nd_step P, int sep0,
                                                      double *__restrict__ linv,
                                                      double *__restrict__ rhs,
                                                      double *__restrict__ y,
                                                      double *__restrict__ status,
                                                      unsigned *__restrict__ kflag,
                                                      unsigned epoch, env_rm R)
{
    const int b = blockIdx.x, np = P.np;
    int t = 0, role;
    if (!P.grouped) {
        while (t + 1 < np && b >= P.b0[t + 1]) t++;
        role = b - P.b0[t];
    } else if (b < np) {   // workgroup 0 of arc b
        t = b;
        role = 0;
    } else if (b < np + P.pb[np]) {   // a panel tile
        const int q = b - np;
        while (t + 1 < np && q >= P.pb[t + 1]) t++;
        role = 1 + q - P.pb[t];
    } else {   // a trailing pair
        const int q = b - np - P.pb[np];
        while (t + 1 < np && q >= P.tb[t + 1]) t++;
        role = 1 + P.T[t] + q - P.tb[t];
    }
    R.kend = P.kend[t];
    if (kflag)
        factor_step_two(S, lds, P.k[t], pan_list + P.pofs[t], P.T[t], pan_list + P.qofs[t],
                        P.Tp[t], linv, rhs, y, status, role, sep0, kflag, epoch, P.ntr[t],
                        P.ts[t], R);
    else
        factor_step_body(S, lds, P.k[t], pan_list + P.pofs[t], P.T[t], pan_list + P.qofs[t],
                         P.Tp[t], linv, rhs, y, status, role, sep0, nullptr, 0);
}

// ---------------------------------------------------------------------------
// k_env_runner: one persistent workgroup per run of columns [k0[t], k1[t])
// (the nested dissection's arcs side by side, or the natural order's one run),
// launched on the side stream beside the per-column launches.  Per column k:
//   A_kk (after its last trailing update: dflag[k] when column k-2 reaches row
//   k) and column k-1's pending update from the workgroup's own LDS copy of
//   L_k,k-1; the factor, L_kk^-1, y_k, published (kflag[k]) exactly as
//   factor_step_two's workgroup 0; then, when row k+1 is in column k's panel,
//   L_k+1,k = A_k+1,k L_kk^-T (after column k-1's panel's r_k+1 update, pflag,
//   and its pending update, uflag) stored with sc1, r_k+1 -= L_k+1,k y_k, lflag[k+1] --
//   the tile stays in LDS for column k+1.  Every tile sees the same operations
//   in the same order as in the column launches alone: bit-identical.  A wait
//   that gives up sets status[1] and ends the workgroup (the host re-solves
//   without hand-offs).
// ---------------------------------------------------------------------------
// (the runs: env_runs, ba_chol_plan.h)
__global__ __launch_bounds__(256) void k_env_runner(double *S, long long lds,
                                                    const int *__restrict__ pan_ptr,
                                                    const int *__restrict__ pan_list, env_runs Rn,
                                                    double *linv, double *rhs, double *y,
                                                    double *status, unsigned *kflag,
                                                    env_rm R, unsigned epoch)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP;
    double *Ls = sm + 2 * NB * LP, *Ps = sm + 3 * NB * LP;
    __shared__ double yk[NB], rk[NB];
    __shared__ double part[4][NB];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (t >= Rn.np) return;
    const int k0 = Rn.k0[t], k1 = Rn.k1[t];
    bool have_l = false;   // Ls holds L_k,k-1
    d4 acc[2][2];
    // row i among column c's panel rows (a wave-wide search, every wave)
    auto reaches = [&](int c, int i) {
        const int q0 = pan_ptr[c], n = pan_ptr[c + 1] - q0;
        bool f = false;
        for (int u = 0; u < n && !f; u += 64) f = __any(u + lane < n && pan_list[q0 + u + lane] == i);
        return f;
    };
    for (int k = k0; k < k1; k++) {
        const int p0 = pan_ptr[k], T = pan_ptr[k + 1] - p0;
        if (k - 2 >= k0 && reaches(k - 2, k) && !env_wait(R.dflag, k, epoch, status, R.rto)) return;
        double vk[16];
        fetch_tile_sc(S, lds, k, k, vk);
        if (tid < NB) rk[tid] = ldg<true>(rhs + (long long)NB * k + tid);
        if (have_l) mfma_64x64(Ls, Ls, acc);
        __syncthreads();
        put_tile(As, vk, false);
        __syncthreads();
        if (have_l) {
            acc_to_lds(acc, As, -1.0, true);
            __syncthreads();
        }
        const bool ok = potrf64_via32(As, Bs, As + 32);
        gemv64(Bs, rk, part, yk, 1.0);   // y_k = L^-1 r_k
        {
            double *lo = linv + (long long)NB * NB * k;
            for (int q = tid; q < NB * NB; q += blockDim.x)
                stg<true>(lo + q, Bs[(q >> 6) * LP + (q & 63)]);
            if (tid < NB) stg<true>(y + (long long)NB * k + tid, yk[tid]);
            if (tid == 0 && !ok) status[0] = 1.0;
        }
        env_publish(kflag, k, epoch);
        have_l = false;
        if (k + 1 < k1 && T > 0 && pan_list[p0] == k + 1) {
            // launch k-1 ended (its trailing update of A_k+1,k and its panel's
            // r_k+1 update), and column k-1's pending update of A_k+1,k stored
            if (k > k0 && reaches(k - 1, k + 1)) {
                // column k-1's panel updated r_k+1; its pending update of A_k+1,k
                if (!env_wait(R.pflag, k + 1, epoch, status, R.rto)) return;
                const bool kin = pan_ptr[k] > pan_ptr[k - 1] && pan_list[pan_ptr[k - 1]] == k;
                if (kin && !env_wait(R.uflag, k + 1, epoch, status, R.rto)) return;
            }
            double va[16];
            fetch_tile_sc(S, lds, k + 1, k, va);
            put_tile(Ps, va, false);
            __syncthreads();
            mfma_64x64(Ps, Bs, acc);   // L[r][c] = sum_t A[r][t] Li[c][t]
            __syncthreads();
            acc_to_lds(acc, Ps, 1.0, false);
            __syncthreads();
            store_tile_sc(S, lds, k + 1, k, Ps);
            double ri[1];
            gemv64(Ps, yk, part, nullptr, 1.0, ri);   // (L y_k)[tid] for tid < 64
            if (tid < NB) {
                double *rp = rhs + (long long)NB * (k + 1) + tid;
                stg<true>(rp, ldg<true>(rp) - ri[0]);
            }
            env_publish(R.lflag, k + 1, epoch);
            double *sw = Ls;
            Ls = Ps;
            Ps = sw;
            have_l = true;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// The arcs' contribution to the separator block (nested dissection): record
// (pair (i, j), arc columns klist[kofs .. kofs+kcnt)) forms
//     P = sum_k L_ik L_jk^T        (and for i == j:  g = sum_k L_ik y_k)
// over its columns in ascending order (one MFMA accumulator chain), stored
// column-major in part[rec][64*64] (+ 64).  Chunks of the arc columns keep
// every record short enough to fill the chip in one wave.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sep_update(const double *__restrict__ S, long long lds,
                                                    const int *__restrict__ pair,
                                                    const int *__restrict__ rec,
                                                    const int *__restrict__ klist,
                                                    const double *__restrict__ y,
                                                    double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP;
    __shared__ double ys[NB];
    const int tid = threadIdx.x, r = tid & 63, cq = tid >> 6;
    const int pr = rec[3 * blockIdx.x], kofs = rec[3 * blockIdx.x + 1], kcnt = rec[3 * blockIdx.x + 2];
    const int i = pair[2 * pr], j = pair[2 * pr + 1];
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int z = 0; z < 2; z++) acc[x][z] = d4{0.0, 0.0, 0.0, 0.0};
    double g = 0.0;   // thread (r, cq): sum over its quarter of the columns
    for (int q = 0; q < kcnt; q++) {
        const int k = klist[kofs + q];
        __syncthreads();   // previous tiles consumed
        load_tile(S, lds, i, k, As);
        if (i != j) load_tile(S, lds, j, k, Bs);
        if (i == j && tid < NB) ys[tid] = y[(long long)NB * k + tid];
        __syncthreads();
        mfma_64x64_acc(As, i == j ? As : Bs, acc);
        if (i == j) {
            double s = 0.0;
#pragma unroll
            for (int c = 16 * cq; c < 16 * cq + 16; c++) s += As[r * LP + c] * ys[c];
            g += s;
        }
    }
    __syncthreads();
    acc_to_lds(acc, As, 1.0, false);
    __syncthreads();
    double *out = part + (size_t)blockIdx.x * (NB * NB + NB);
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int c = cq + 4 * u;
        out[c * NB + r] = As[r * LP + c];
    }
    if (i == j) {
        __shared__ double gp[4][NB];
        gp[cq][r] = g;
        __syncthreads();
        if (tid < NB) out[NB * NB + tid] = ((gp[0][tid] + gp[1][tid]) + gp[2][tid]) + gp[3][tid];
    }
}

// A_ij -= sum of the pair's records (in record order); rhs_i -= sum of g
__global__ __launch_bounds__(256) void k_sep_reduce(double *__restrict__ S, long long lds,
                                                    const int *__restrict__ pair,
                                                    const int *__restrict__ pptr,
                                                    const double *__restrict__ part,
                                                    double *__restrict__ rhs)
{
    const int p = blockIdx.x, tid = threadIdx.x, r = tid & 63, cq = tid >> 6;
    const int i = pair[2 * p], j = pair[2 * p + 1];
    const int e0 = pptr[p], e1 = pptr[p + 1];
    double s[16];
#pragma unroll
    for (int u = 0; u < 16; u++) s[u] = 0.0;
    double g = 0.0;
    for (int e = e0; e < e1; e++) {
        const double *src = part + (size_t)e * (NB * NB + NB);
#pragma unroll
        for (int u = 0; u < 16; u++) s[u] += src[(cq + 4 * u) * NB + r];
        if (i == j && tid < NB) g += src[NB * NB + tid];
    }
    double *base = S + (long long)NB * i + lds * (long long)NB * j;
#pragma unroll
    for (int u = 0; u < 16; u++) base[r + lds * (cq + 4 * u)] -= s[u];
    if (i == j && tid < NB) rhs[(long long)NB * i + tid] -= g;
}

// da (camera order, ld..lds zero) from the row-ordered solution
__global__ void k_nd_scatter(const int *__restrict__ prow, const double *__restrict__ x,
                             double *__restrict__ da, long long lds)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= lds) return;
    const int r = prow[c];
    da[c] = r >= 0 ? x[r] : 0.0;
}

// ---------------------------------------------------------------------------
// backward solve step k: x_k = L_kk^-T z_k; z_j -= L_kj^T x_k, j in [j0, k)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_backward(const double *__restrict__ S, long long lds,
                                                  int k, int j0,
                                                  const double *__restrict__ linv,
                                                  double *__restrict__ z, double *__restrict__ x)
{
    __shared__ double xs[NB], zk[NB];
    __shared__ double part[4][NB];
    __shared__ double Lt[NB * LP];
    const int j = j0 + blockIdx.x, tid = threadIdx.x;
    const double *lo = linv + (long long)NB * NB * k;  // row-major L^-1
    load_rowmajor(lo, Lt);
    if (tid < NB) zk[tid] = z[(long long)NB * k + tid];
    __syncthreads();
    {   // x_k[c] = sum_{r >= c} Li[r][c] z_k[r]: thread (c, quarter)
        const int c = tid & 63, qr = tid >> 6;
        double s = 0.0;
        for (int r = 16 * qr; r < 16 * qr + 16; r++)
            if (r >= c) s += Lt[r * LP + c] * zk[r];
        part[qr][c] = s;
    }
    __syncthreads();
    if (tid < NB) xs[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    __syncthreads();
    if (j == k) {
        if (tid < NB) x[(long long)NB * k + tid] = xs[tid];
        return;
    }
    // z_j[c] -= sum_r L_kj[r][c] x_k[r]: stage L_kj (coalesced), thread (c, quarter)
    load_tile(S, lds, k, j, Lt);
    __syncthreads();
    const int c = tid & 63, qr = tid >> 6;
    double s = 0.0;
#pragma unroll
    for (int r = 16 * qr; r < 16 * qr + 16; r++) s += Lt[r * LP + c] * xs[r];
    part[qr][c] = s;
    __syncthreads();
    if (tid < NB)
        z[(long long)NB * j + tid] -= ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ---------------------------------------------------------------------------
// The envelope's backward solve in ONE launch (the per-column k_backward
// launches sat at the launch floor).  Workgroup w takes tile column
// j = nt-1-w (top first): z_j = y_j - sum over the envelope rows k > j (k
// descending, the order of the per-column launches: bit-identical) of
// L_kj^T x_k, then x_j = L_jj^-T z_j, published as 128 epoch-tagged 8-byte
// write-through granules (cdna_hip_programming.md Guideline 16, R2); each x_k
// is swept by wave 0 until every tag matches.  Used when every column is
// co-resident (one workgroup per CU by LDS: nt <= CUs); a spin that never
// ends sets the timeout word status[1] instead of hanging.  Each tile (k, j) is loaded while
// the wave waits for x_k.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_backward_all(const double *__restrict__ S, long long lds,
                                                      int nt, const int *__restrict__ pan_ptr,
                                                      const int *__restrict__ pan,
                                                      const double *__restrict__ linv,
                                                      const double *__restrict__ z,
                                                      double *__restrict__ x,
                                                      unsigned long long *__restrict__ xg,
                                                      unsigned epoch, double *status)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *Lt = sm, *Li = sm + NB * LP;
    __shared__ __attribute__((aligned(16))) double zj[NB], xs[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = nt - 1 - (int)blockIdx.x;
    load_rowmajor(linv + (long long)NB * NB * j, Li);
    if (tid < NB) zj[tid] = z[(long long)NB * j + tid];
    const int c = tid & 63, qr = tid >> 6;
    for (int idx = pan_ptr[j + 1] - 1; idx >= pan_ptr[j]; idx--) {
        const int k = pan[idx];
        __syncthreads();   // Lt / xs of the previous k consumed
        load_tile(S, lds, k, j, Lt);
        if (wv == 0) {
            const unsigned long long *g = xg + 128 * (size_t)k;
            unsigned long long v0 = 0, v1 = 0;
            for (unsigned spins = 0;; spins++) {
                v0 = __hip_atomic_load(g + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v1 = __hip_atomic_load(g + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((unsigned)(v0 >> 32) == epoch && (unsigned)(v1 >> 32) == epoch)) break;
                if (spins >= BA_BACK_SPIN_MAX) {
                    if (lane == 0) status[1] = 1.0;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            unsigned *xu = reinterpret_cast<unsigned *>(xs);
            xu[lane] = (unsigned)v0;
            xu[64 + lane] = (unsigned)v1;
        }
        __syncthreads();
        // z_j[c] -= sum_r L_kj[r][c] x_k[r]: thread (c, quarter), as k_backward
        double s = 0.0;
#pragma unroll
        for (int r = 16 * qr; r < 16 * qr + 16; r++) s += Lt[r * LP + c] * xs[r];
        part[qr][c] = s;
        __syncthreads();
        if (tid < NB) zj[tid] -= ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    }
    __syncthreads();
    {   // x_j[c] = sum_{r >= c} Li[r][c] z_j[r]: thread (c, quarter), as k_backward
        double s = 0.0;
        for (int r = 16 * qr; r < 16 * qr + 16; r++)
            if (r >= c) s += Li[r * LP + c] * zj[r];
        part[qr][c] = s;
    }
    __syncthreads();
    if (tid < NB) {
        const double xv = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        xs[tid] = xv;
        x[(long long)NB * j + tid] = xv;
    }
    __syncthreads();
    if (wv == 0) {
        const unsigned *xu = reinterpret_cast<const unsigned *>(xs);
        unsigned long long *g = xg + 128 * (size_t)j;
        __hip_atomic_store(g + lane, ((unsigned long long)epoch << 32) | xu[lane],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(g + 64 + lane, ((unsigned long long)epoch << 32) | xu[64 + lane],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// Block cyclic reduction for a tile-tridiagonal S (co-visibility band narrower
// than one tile: tile row i couples only with tiles i-1, i+1).  This is the
// Cholesky factorisation of S in odd-even (nested-dissection) order: at each
// level the even positions e of the active tile list are eliminated in
// parallel; their neighbours p < e < q are kept and coupled through e.  Per
// eliminated tile e (L_e = chol(D_e)):
//     Lp_e = L(p, e) = C(p, e) L_e^-T,   Lq_e = L(q, e) = C(q, e) L_e^-T,
//     y_e  = L_e^-1 r_e
// per kept tile k with eliminated neighbours e- < k < e+ and next kept k2:
//     D_k -= Lq_{e-} Lq_{e-}^T + Lp_{e+} Lp_{e+}^T,
//     r_k -= Lq_{e-} y_{e-} + Lp_{e+} y_{e+},
//     C(k2, k) = -Lq_{e+} Lp_{e+}^T          (fill between the kept tiles)
// log2(nt) levels instead of nt sequential tile steps.  Back substitution in
// reverse level order: x_e = L_e^-T (y_e - Lp_e^T x_p - Lq_e^T x_q).
// C(i, j), i > j, lives in S tile (i, j); Lp / Lq in crL[2][nt][64*64].
// ---------------------------------------------------------------------------
// Rows 32h .. 32h+31 of the 64x64 product acc = As[r][:] . Bs[c][:] (K = 64):
// wave w owns rows 32h + 16(w>>1) .. +15, cols 32(w&1) .. +31 (two 16x16
// MFMA tiles), half the MFMA chain of mfma_64x64.
__device__ __forceinline__ void mfma_half(const double *As, const double *Bs, int h, d4 acc[2],
                                          bool zero)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * h + 16 * (w >> 1), c0 = 32 * (w & 1);
    const int li = lane & 15, lk = lane >> 4;
    if (zero) acc[0] = acc[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < NB / 4; s++) {
        const int kk = 4 * s + lk;
        const double a0 = As[(r0 + li) * LP + kk];
        const double b0 = Bs[(c0 + li) * LP + kk];
        const double b1 = Bs[(c0 + 16 + li) * LP + kk];
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
    }
}

// mfma_half's result: T[r][c] = scale * acc (+ T[r][c] if add)
__device__ __forceinline__ void half_to_lds(const d4 acc[2], double *T, int h, double scale,
                                            bool add)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * h + 16 * (w >> 1), c0 = 32 * (w & 1);
#pragma unroll
    for (int y = 0; y < 2; y++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = r0 + (lane >> 4) + 4 * q, c = c0 + 16 * y + (lane & 15);
            const double v = scale * acc[y][q];
            T[r * LP + c] = add ? T[r * LP + c] + v : v;
        }
}

// rows 32h .. +31 of LDS T[r][c] -> row-major dst[r*64 + c]
__device__ __forceinline__ void store_rowmajor_half(double *__restrict__ dst, const double *T,
                                                    int h)
{
    const int c = threadIdx.x & 63, r0 = 32 * h + (threadIdx.x >> 6);
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = T[(r0 + 4 * u) * LP + c];
#pragma unroll
    for (int u = 0; u < 8; u++) dst[(r0 + 4 * u) * NB + c] = v[u];
}

// rows 32h .. +31 of S tile (ti, tj) <-> LDS T[r][c]; thread (row, 8 columns)
__device__ __forceinline__ void load_tile_half(const double *__restrict__ S, long long lds, int ti,
                                               int tj, double *T, int h)
{
    const double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = 32 * h + (threadIdx.x & 31), c0 = threadIdx.x >> 5;
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = base[r + lds * (c0 + 8 * u)];
#pragma unroll
    for (int u = 0; u < 8; u++) T[r * LP + c0 + 8 * u] = v[u];
}

__device__ __forceinline__ void store_tile_half(double *__restrict__ S, long long lds, int ti,
                                                int tj, const double *T, int h)
{
    double *base = S + (long long)NB * ti + lds * (long long)NB * tj;
    const int r = 32 * h + (threadIdx.x & 31), c0 = threadIdx.x >> 5;
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = T[r * LP + c0 + 8 * u];
#pragma unroll
    for (int u = 0; u < 8; u++) base[r + lds * (c0 + 8 * u)] = v[u];
}

// Factor step of a level.  split = 0: one workgroup per eliminated tile does
// everything.  split = 1 (levels narrow enough that 5 workgroups per tile fit
// the chip): workgroup role 0 factors D_e and writes L_e^-1 and y_e; roles
// 1-2 (rows halves of Lp_e) and 3-4 (of Lq_e) redo the same factorisation --
// deterministic, bit-identical -- with their C tile loaded alongside, and form
// their 32 rows of the panel.  The critical path loses both 64x64 panel GEMMs.
__global__ __launch_bounds__(256) void k_cr_factor(double *__restrict__ S, long long lds,
                                                   const int *__restrict__ elim, int nt,
                                                   double *__restrict__ linv,
                                                   double *__restrict__ crL,
                                                   const double *__restrict__ rhs,
                                                   double *__restrict__ y,
                                                   double *__restrict__ status, int split)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP, *Cs = sm + 2 * NB * LP;
    __shared__ double rk[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x;
    const int x = split ? blockIdx.x / 5 : blockIdx.x, role = split ? blockIdx.x % 5 : -1;
    const int e = elim[3 * x], p = elim[3 * x + 1], q = elim[3 * x + 2];
    if ((role == 1 || role == 2) && p < 0) return;
    if ((role == 3 || role == 4) && q < 0) return;
    {
        double va[16], vc[16];
        fetch_tile(S, lds, e, e, va);
        if (role > 0) {   // C(p, e) = tile(e, p)^T  |  C(q, e) = tile(q, e)
            if (role <= 2)
                fetch_tile(S, lds, e, p, vc);
            else
                fetch_tile(S, lds, q, e, vc);
        }
        if (role <= 0 && tid < NB) rk[tid] = rhs[(long long)NB * e + tid];
        put_tile(As, va, false);
        if (role > 0) put_tile(Cs, vc, role <= 2);
    }
    __syncthreads();
    const bool ok = block_potrf_inv(As, Bs, false);
    if (role > 0) {
        const int h = (role - 1) & 1;
        d4 acc[2];
        mfma_half(Cs, Bs, h, acc, true);
        __syncthreads();
        half_to_lds(acc, Cs, h, 1.0, false);
        __syncthreads();
        store_rowmajor_half(crL + (long long)NB * NB * (role <= 2 ? e : nt + e), Cs, h);
        return;
    }
    gemv64(Bs, rk, part, y + (long long)NB * e, 1.0);
    store_rowmajor(linv + (long long)NB * NB * e, Bs);
    if (tid == 0 && !ok) status[0] = 1.0;
    if (split) return;
    d4 acc[2][2];
    if (p >= 0) {   // C(p, e) = tile(e, p)^T
        load_tile_t(S, lds, e, p, Cs);
        __syncthreads();
        mfma_64x64(Cs, Bs, acc);
        __syncthreads();
        acc_to_lds(acc, Cs, 1.0, false);
        __syncthreads();
        store_rowmajor(crL + (long long)NB * NB * e, Cs);
        __syncthreads();
    }
    if (q >= 0) {   // C(q, e) = tile(q, e)
        load_tile(S, lds, q, e, Cs);
        __syncthreads();
        mfma_64x64(Cs, Bs, acc);
        __syncthreads();
        acc_to_lds(acc, Cs, 1.0, false);
        __syncthreads();
        store_rowmajor(crL + (long long)NB * NB * (nt + e), Cs);
    }
}

// Update step of a level.  split = 0: one workgroup per kept tile.  split = 1:
// four workgroups per kept tile -- roles 0/1 update rows halves of D_k (role 0
// also r_k), roles 2/3 form rows halves of the fill C(k2, k).
__global__ __launch_bounds__(256) void k_cr_update(double *__restrict__ S, long long lds,
                                                   const int *__restrict__ keep, int nt,
                                                   const double *__restrict__ crL,
                                                   double *__restrict__ rhs,
                                                   const double *__restrict__ y, int split)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *As = sm, *Bs = sm + NB * LP, *Cs = sm + 2 * NB * LP;
    __shared__ double ym[NB], yp[NB], um[NB], up[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x;
    const int x = split ? blockIdx.x >> 2 : blockIdx.x, role = split ? blockIdx.x & 3 : -1;
    const int *kp = keep + 4 * x;
    const int k = kp[0], em = kp[1], ep = kp[2], k2 = kp[3];
    const long long T2 = (long long)NB * NB;
    if (role >= 2) {   // C(k2, k) = -Lq_{e+} Lp_{e+}^T, rows half role - 2
        if (k2 < 0) return;
        const int h = role - 2;
        load_rowmajor(crL + T2 * (nt + ep), Bs);
        load_rowmajor(crL + T2 * ep, Cs);
        __syncthreads();
        d4 acc[2];
        mfma_half(Bs, Cs, h, acc, true);
        half_to_lds(acc, As, h, -1.0, false);
        __syncthreads();
        store_tile_half(S, lds, k2, k, As, h);
        return;
    }
    if (role >= 0) {   // rows half `role` of D_k
        const int h = role;
        load_tile_half(S, lds, k, k, As, h);
        load_rowmajor(crL + T2 * (nt + em), Bs);   // Lq_{e-} = L(k, e-)
        if (ep >= 0) load_rowmajor(crL + T2 * ep, Cs);   // Lp_{e+} = L(k, e+)
        if (h == 0 && tid < NB) {
            ym[tid] = y[(long long)NB * em + tid];
            yp[tid] = (ep >= 0) ? y[(long long)NB * ep + tid] : 0.0;
        }
        __syncthreads();
        d4 acc[2];
        mfma_half(Bs, Bs, h, acc, true);
        if (ep >= 0) mfma_half(Cs, Cs, h, acc, false);
        half_to_lds(acc, As, h, -1.0, true);   // each thread updates the elements it owns
        if (h == 0) {
            gemv64(Bs, ym, part, um, 1.0);
            if (ep >= 0) gemv64(Cs, yp, part, up, 1.0);
            if (tid < NB) {
                double r = rhs[(long long)NB * k + tid] - um[tid];
                if (ep >= 0) r -= up[tid];
                rhs[(long long)NB * k + tid] = r;
            }
        }
        __syncthreads();
        store_tile_half(S, lds, k, k, As, h);
        return;
    }
    load_tile(S, lds, k, k, As);
    load_rowmajor(crL + T2 * (nt + em), Bs);   // Lq_{e-} = L(k, e-)
    if (ep >= 0) load_rowmajor(crL + T2 * ep, Cs);   // Lp_{e+} = L(k, e+)
    if (tid < NB) {
        ym[tid] = y[(long long)NB * em + tid];
        yp[tid] = (ep >= 0) ? y[(long long)NB * ep + tid] : 0.0;
    }
    __syncthreads();
    d4 acc[2][2];
    mfma_64x64(Bs, Bs, acc);
    if (ep >= 0) mfma_64x64_acc(Cs, Cs, acc);
    acc_to_lds(acc, As, -1.0, true);   // each thread updates the elements it owns
    gemv64(Bs, ym, part, um, 1.0);
    if (ep >= 0) gemv64(Cs, yp, part, up, 1.0);
    if (tid < NB) {
        double r = rhs[(long long)NB * k + tid] - um[tid];
        if (ep >= 0) r -= up[tid];
        rhs[(long long)NB * k + tid] = r;
    }
    __syncthreads();
    store_tile(S, lds, k, k, As);
    if (k2 >= 0) {   // C(k2, k) = -Lq_{e+} Lp_{e+}^T
        __syncthreads();
        load_rowmajor(crL + T2 * (nt + ep), Bs);
        __syncthreads();
        mfma_64x64(Bs, Cs, acc);
        __syncthreads();
        acc_to_lds(acc, As, -1.0, false);
        __syncthreads();
        store_tile(S, lds, k2, k, As);
    }
}


// LDS of one cyclic-reduction record: five 32-row tiles, the 16-row scratch
// of potrf32_inv, five 32-vectors and the gemv partials.  The per-level
// kernels declare it as static LDS; k_cr32_fused carves every record type
// (factor, fused level, survivor, back substitution) from one pool of this
// shape (96 KB: one workgroup per CU, which its hand-offs rely on).
struct cr32_lds {
    double *As, *Bs, *Cs, *Ds, *Es, *Xs;
    double *rk, *ym, *yp, *um, *up;
    double (*part)[T32];
};

#define CR32_LDS_DECL                                                                      \
    __shared__ __attribute__((aligned(16))) double cr_As[T32 * LP], cr_Bs[T32 * LP],      \
        cr_Cs[T32 * LP], cr_Ds[T32 * LP], cr_Es[T32 * LP];                                 \
    __shared__ __attribute__((aligned(16))) double cr_Xs[16 * LP];                         \
    __shared__ __attribute__((aligned(16))) double cr_v[5][T32];                           \
    __shared__ __attribute__((aligned(16))) double cr_part[8][T32];                        \
    const cr32_lds sh{cr_As, cr_Bs, cr_Cs, cr_Ds, cr_Es, cr_Xs, cr_v[0], cr_v[1], cr_v[2], \
                      cr_v[3], cr_v[4], cr_part}

// Diagnostic build only (make stamps): per record of k_cr32_fused, the
// s_memrealtime (100 MHz) at entry, after its wait, before and after its
// publish, and inside the record bodies (SC instantiation only): [4] loads
// in LDS, [5] update applied, [6] factor + panel done, [7] before the panel
// store; [8] / [9] cr32_chol's first pivot chain / MFMA stage done
// (tools/cr_timeline.py)
#ifdef BA_STAMPS
#define CR_ST_MAX 8192
__device__ unsigned long long g_crst[CR_ST_MAX][12];
extern "C" int vlgba_debug_crstamps(unsigned long long *out, int nrec)
{
    if (nrec > CR_ST_MAX) nrec = CR_ST_MAX;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_crst), sizeof(unsigned long long) * 12 * nrec) ==
                   hipSuccess
               ? 0
               : -1;
}
#define CR_ST(k)                                                                          \
    do {                                                                                  \
        if (threadIdx.x == 0 && blockIdx.x < CR_ST_MAX)                                   \
            g_crst[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();                     \
    } while (0)
#define CR_SUB(k)                                                                         \
    do {                                                                                  \
        if constexpr (SC)                                                                 \
            if (threadIdx.x == 0 && blockIdx.x < CR_ST_MAX)                               \
                g_crst[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();                 \
    } while (0)
#else
#define CR_ST(k)
#define CR_SUB(k)
#endif

// factor step (level 0, on the assembled S): role 0 factors D_e, writes L_e^-1
// (row-major 32 x 32) and y_e = L_e^-1 r_e; role 1 / 2 (split, one workgroup
// each, redoing the same factorisation) form Lp_e = C(p, e) L_e^-T / Lq_e =
// C(q, e) L_e^-T into crL (the panel rides on the factor: cr32_chol); role 4
// = roles 0 and 1 in one workgroup (y by a GEMV with L^-1 there: the panel
// takes the factor's spare lanes); role -1 (no split) = role 4, then the
// factorisation again for the q panel (the same operations as role 2, so the
// split and unsplit launches agree bit for bit).
template <bool SC>
__device__ __forceinline__ void cr32_factor_body(const cr32_lds &sh, double *S, long long lds,
                                                 int TB, long long ld, int e, int p, int q,
                                                 int role, int nt, double *linv, double *crL,
                                                 const double *rhs, double *y, double *status)
{
    double *As = sh.As, *Bs = sh.Bs, *Cs = sh.Cs, *Xs = sh.Xs, *rk = sh.rk, *yk = sh.ym;
    const int tid = threadIdx.x;
    const long long T2 = (long long)T32 * T32;
    const bool rows = role <= 0 || role == 4;
    const int side = role == 2 ? 2 : 1;   // the panel of this pass (role 0: none)
    const bool pan = (role == 1 || role == 4 || role < 0) ? p >= 0 : (role == 2 && q >= 0);
    load32<SC>(S, lds, TB, ld, e, e, As, false, true);
    if (pan && side == 1) load32<SC>(S, lds, TB, ld, e, p, Cs, true, false);   // C(p, e) = tile(e, p)^T
    if (pan && side == 2) load32<SC>(S, lds, TB, ld, q, e, Cs, false, false);  // C(q, e) = tile(q, e)
    if (rows && tid < T32) {
        const long long g = (long long)TB * e + tid;
        rk[tid] = (tid < TB && g < ld) ? ldg<SC>(rhs + g) : 0.0;
    }
    __syncthreads();
    CR_SUB(4);
    CR_SUB(5);
    // y rides on the factor's spare lanes unless a panel fills them (roles 4, -1)
    const bool ylanes = rows && !pan;
    const bool ok = cr32_chol(As, rows ? Bs : nullptr, pan ? Cs : nullptr, Xs,
                              ylanes ? rk : nullptr, yk, [](int) {});
    CR_SUB(6);
    if (pan) {
        CR_SUB(7);
        store_rm32<SC>(crL + T2 * (side == 1 ? e : nt + e), Cs);
    }
    if (rows) {
        if (!ylanes) gemv32(Bs, rk, sh.part, yk, false);
        if (tid < TB) stg<SC>(y + (long long)TB * e + tid, yk[tid]);
        store_rm32<SC>(linv + T2 * e, Bs);
        if (tid == 0 && !ok) status[0] = 1.0;
    }
    if (role < 0 && q >= 0) {   // unsplit: the q panel (role 2's pass)
        __syncthreads();
        load32<SC>(S, lds, TB, ld, e, e, As, false, true);
        load32<SC>(S, lds, TB, ld, q, e, Cs, false, false);
        __syncthreads();
        cr32_chol(As, nullptr, Cs, Xs, nullptr, nullptr, [](int) {});
        store_rm32<SC>(crL + T2 * (nt + e), Cs);
    }
}

__global__ __launch_bounds__(256) void k_cr32_factor(double *__restrict__ S, long long lds,
                                                     int TB, long long ld,
                                                     const int *__restrict__ elim, int nt,
                                                     double *__restrict__ linv,
                                                     double *__restrict__ crL,
                                                     const double *__restrict__ rhs,
                                                     double *__restrict__ y,
                                                     double *__restrict__ status, int split)
{
    __shared__ __attribute__((aligned(16))) double As[T32 * LP], Bs[T32 * LP], Cs[T32 * LP];
    __shared__ __attribute__((aligned(16))) double Xs[16 * LP];
    __shared__ double rk[T32], yk[T32];
    __shared__ double part[8][T32];
    const cr32_lds sh{As, Bs, Cs, nullptr, nullptr, Xs, rk, yk, nullptr, nullptr, nullptr, part};
    const int x = split ? blockIdx.x / 3 : blockIdx.x, role = split ? blockIdx.x % 3 : -1;
    const int e = elim[3 * x], p = elim[3 * x + 1], q = elim[3 * x + 2];
    if ((role == 1 && p < 0) || (role == 2 && q < 0)) return;
    cr32_factor_body<false>(sh, S, lds, TB, ld, e, p, q, role, nt, linv, crL, rhs, y, status);
}

// Level L >= 1 of the camera-aligned CR with the previous level's update folded
// in (one launch per level instead of two).  Tile k of level L carries the
// update of level L-1,
//     D_k -= L(k, em) L(k, em)^T + L(k, ep) L(k, ep)^T,  r_k -= L(k, em) y_em + L(k, ep) y_ep
// (em / ep: the tiles eliminated at L-1 next to k), and the coupling of two
// neighbours k < k2 at level L is the fill C(k2, k) = -L(k2, e) L(k, e)^T of
// the tile e eliminated between them.  Workgroups 3x + role for the tiles
// eliminated here (role 0: apply the update, factor, y, L^-1; roles 1 / 2:
// the same factorisation with their fill tile C(p, e) / C(q, e) as the panel
// rows of cr32_chol), then one workgroup per surviving tile (role 3: apply
// the update, write D_k back, mid(), then r_k).  Records: fused (e, p, q,
// em, ep), survivor (k, em, ep).  The eliminated tiles' update is split by
// 16 x 16 block: D00 and D10 (and the fill's first 16 columns) before the
// first pivot chain, D11 and the rest of the fill beside it (cr32_chol's
// side); role 0's r update runs beside the D00 / D10 blocks.  mid: the
// survivor's D_k is published before its r_k (k_cr32_fused: the panel roles
// of the next level need only D_k, and r_k waits for the neighbours' y).
// r_k -= L(k, em) y_em + L(k, ep) y_ep by one wave: lane r < 32 row r of the
// first product, lane 32 + r of the second, each a sequential sum over the
// 32 columns.
__device__ __forceinline__ void cr32_rupd(const double *Bs, const double *Cs, bool two,
                                          const double *ym, const double *yp, double *rk,
                                          double *up)
{
    const int lane = threadIdx.x & 63, r = lane & 31;
    const double *M = lane < 32 ? Bs : Cs;
    const double *v = lane < 32 ? ym : yp;
    double t = 0.0;
#pragma unroll
    for (int c = 0; c < T32; c++) t = fma(M[r * LP + c], v[c], t);
    if (lane >= 32) up[r] = two ? t : 0.0;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < 32) rk[r] = (rk[r] - t) - up[r];
}

// The one-launch CR's per-wave operand hand-off (k_cr32_fused, level L >= 1):
// each wave polls only the flags of the operand it loads and loads it at once
// (all 64 lanes, sc1), so an operand whose producer finished early is in LDS
// while the wave of a later one still waits; one barrier after all of them.
// The union of the waves' flags is the record's former flag set.
struct cr32_pw {
    const unsigned *flag;
    unsigned epoch;
    double *status;
    int L, nt;
};

__device__ __forceinline__ void cr32_wave_wait(const cr32_pw &pw, const int *w, int nw)
{
    const int lane = threadIdx.x & 63;
    int idx = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (lane == q && q < nw) idx = w[q];
    for (unsigned spins = 0;; spins++) {
        const bool ok = lane >= nw || __hip_atomic_load((const gu32_t *)(pw.flag + idx),
                                                        __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT) == pw.epoch;
        if (__all(ok)) break;
        if (spins >= BA_BACK_SPIN_MAX) {
            if (lane == 0) pw.status[1] = 1.0;
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

template <bool SC, class Mid>
__device__ __forceinline__ void cr32_level_body(const cr32_lds &sh, double *S, long long lds,
                                                int TB, long long ld, int k, int p, int q, int em,
                                                int ep, int role, int nt, double *linv,
                                                double *crL, double *rhs, double *y,
                                                double *status, Mid mid,
                                                const cr32_pw *pw = nullptr)
{
    double *As = sh.As, *Bs = sh.Bs, *Cs = sh.Cs, *Ds = sh.Ds, *Es = sh.Es, *Xs = sh.Xs;
    double *rk = sh.rk, *ym = sh.ym, *yp = sh.yp, *um = sh.um, *up = sh.up;
    const int tid = threadIdx.x, w = tid >> 6;
    const long long T2 = (long long)T32 * T32;
    const bool surv = role == 3;
    auto load_r = [&]() {
        if (tid < T32) {
            const long long g = (long long)TB * k + tid;
            rk[tid] = (tid < TB && g < ld) ? ldg<SC>(rhs + g) : 0.0;
            ym[tid] = tid < TB ? ldg<SC>(y + (long long)TB * em + tid) : 0.0;
            yp[tid] = (ep >= 0 && tid < TB) ? ldg<SC>(y + (long long)TB * ep + tid) : 0.0;
        }
    };
    if (SC && pw) {   // per wave: its operand's flags, then its operand
        auto fw = [&](int t, int r) { return 5 * ((pw->L - 1) * nt + t) + r; };
        const bool own = pw->L >= 2;
        int wl[4], n = 0;
        if (w == 0) {          // D_k (its survivor record at L - 1)
            if (own) {
                wl[n++] = fw(k, 3);
                if (role == 0) wl[n++] = fw(k, 4);
            }
            cr32_wave_wait(*pw, wl, n);
            load32_wave(S, lds, TB, ld, k, k, As, false, true);
        } else if (w == 1) {   // L(k, em) = role 2 of em (role 0 waits for all of em)
            wl[n++] = fw(em, 2);
            if (role == 0 || role == 1) wl[n++] = fw(em, 1);
            if (role == 0) wl[n++] = fw(em, 0);
            cr32_wave_wait(*pw, wl, n);
            load_rm32_wave(crL + T2 * (nt + em), Bs);
        } else if (w == 2) {   // L(k, ep) = role 1 of ep
            if (ep >= 0) {
                wl[n++] = fw(ep, 1);
                if (role == 0 || role == 2) wl[n++] = fw(ep, 2);
                if (role == 0) wl[n++] = fw(ep, 0);
                cr32_wave_wait(*pw, wl, n);
                load_rm32_wave(crL + T2 * ep, Cs);
            }
        } else if (role == 1 || role == 2) {   // the fill's L(p, em) | L(q, ep)
            wl[n++] = role == 1 ? fw(em, 1) : fw(ep, 2);
            cr32_wave_wait(*pw, wl, n);
            load_rm32_wave(crL + T2 * (role == 1 ? em : nt + ep), Ds);
        } else if (role == 0) {   // r_k, y_em, y_ep on this wave's first 32 lanes
            wl[n++] = fw(em, 0);
            if (ep >= 0) wl[n++] = fw(ep, 0);
            if (own) wl[n++] = fw(k, 4);
            cr32_wave_wait(*pw, wl, n);
            const int i = tid & 63;
            if (i < T32) {
                const long long g = (long long)TB * k + i;
                rk[i] = (i < TB && g < ld) ? ldg<SC>(rhs + g) : 0.0;
                ym[i] = i < TB ? ldg<SC>(y + (long long)TB * em + i) : 0.0;
                yp[i] = (ep >= 0 && i < TB) ? ldg<SC>(y + (long long)TB * ep + i) : 0.0;
            }
        }
        __syncthreads();
    } else {
        load32<SC>(S, lds, TB, ld, k, k, As, false, true);
        load_rm32<SC>(crL + T2 * (nt + em), Bs);            // L(k, em)
        if (ep >= 0) load_rm32<SC>(crL + T2 * ep, Cs);      // L(k, ep)
        if (role == 1) load_rm32<SC>(crL + T2 * em, Ds);    // L(p, em)
        if (role == 2) load_rm32<SC>(crL + T2 * (nt + ep), Ds);   // L(q, ep)
        if (role == 0) load_r();
        __syncthreads();
    }
    CR_SUB(4);
    if (surv) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma32_nt(Bs, Bs, acc);
        if (ep >= 0) acc = mfma32_nt(Cs, Cs, acc);
        put32(As, acc, -1.0, true);   // each thread updates the elements it owns
        __syncthreads();
        store32<SC>(S, lds, TB, ld, k, k, As);
        mid();
        load_r();
        __syncthreads();
        if (w == 0) cr32_rupd(Bs, Cs, ep >= 0, ym, yp, rk, up);
        __syncthreads();
        if (tid < TB) {
            const long long g = (long long)TB * k + tid;
            if (g < ld) stg<SC>(rhs + g, rk[tid]);
        }
        return;
    }
    const double *G = role == 2 ? Cs : Bs;   // the fill's right factor: L(k, em) | L(k, ep)
    // block (ri, ci) of D -= Lm Lm^T + Lp Lp^T (K = 32 each)
    auto dupd = [&](int ri, int ci) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = mfma16_nt(Bs, ri, 0, Bs, ci, 0, acc);
        acc = mfma16_nt(Bs, ri, 16, Bs, ci, 16, acc);
        if (ep >= 0) {
            acc = mfma16_nt(Cs, ri, 0, Cs, ci, 0, acc);
            acc = mfma16_nt(Cs, ri, 16, Cs, ci, 16, acc);
        }
        put16(As, ri, ci, acc, -1.0, true);
    };
    // block (ri, ci) of the fill: Es = -Ds G^T
    auto fill = [&](int ri, int ci) {
        d4 f = {0.0, 0.0, 0.0, 0.0};
        f = mfma16_nt(Ds, ri, 0, G, ci, 0, f);
        f = mfma16_nt(Ds, ri, 16, G, ci, 16, f);
        put16(Es, ri, ci, f, -1.0, false);
    };
    const bool pan = role != 0;
    if (w == 0)
        dupd(0, 0);
    else if (w == 1)
        dupd(16, 0);
    else if (pan)
        fill(16 * (w - 2), 0);
    else if (w == 2)
        cr32_rupd(Bs, Cs, ep >= 0, ym, yp, rk, up);
    __syncthreads();
    CR_SUB(5);
    const bool ok = cr32_chol(As, pan ? nullptr : Ds, pan ? Es : nullptr, Xs, pan ? nullptr : rk,
                              um, [&](int ww) {
                                  if (ww == 1)
                                      dupd(16, 16);
                                  else if (pan)
                                      fill(16 * (ww - 2), 16);
                              });
    CR_SUB(6);
    if (role == 0) {   // L^-1 in Ds (no fill for role 0), y in um
        if (tid < TB) stg<SC>(y + (long long)TB * k + tid, um[tid]);
        store_rm32<SC>(linv + T2 * k, Ds);
        if (tid == 0 && !ok) status[0] = 1.0;
        return;
    }
    CR_SUB(7);
    store_rm32<SC>(crL + T2 * (role == 1 ? k : nt + k), Es);
}

__global__ __launch_bounds__(256) void k_cr32_level(double *__restrict__ S, long long lds, int TB,
                                                    long long ld, const int *__restrict__ frec,
                                                    int ne, const int *__restrict__ srec, int nt,
                                                    double *__restrict__ linv,
                                                    double *__restrict__ crL,
                                                    double *__restrict__ rhs,
                                                    double *__restrict__ y,
                                                    double *__restrict__ status)
{
    CR32_LDS_DECL;
    const bool surv = (int)blockIdx.x >= 3 * ne;
    int k, p = -1, q = -1, em, ep, role = 3;
    if (surv) {
        const int *r = srec + 3 * (blockIdx.x - 3 * ne);
        k = r[0];
        em = r[1];
        ep = r[2];
    } else {
        const int *r = frec + 5 * (blockIdx.x / 3);
        role = blockIdx.x % 3;
        k = r[0];
        p = r[1];
        q = r[2];
        em = r[3];
        ep = r[4];
        if ((role == 1 && p < 0) || (role == 2 && q < 0)) return;
    }
    cr32_level_body<false>(sh, S, lds, TB, ld, k, p, q, em, ep, role, nt, linv, crL, rhs, y,
                           status, [] {});
}

// Back substitution of one eliminated tile e (neighbours p, q):
//     x_e = L_e^-T (y_e - Lp_e^T x_p - Lq_e^T x_q) = z_e - Mp x_p - Mq x_q,
//     z_e = L_e^-T y_e,  Mp = L_e^-T Lp_e^T,  Mq = L_e^-T Lq_e^T.
// z, Mp and Mq need only the factor step's outputs, so they are formed
// before the neighbours' x is fetched (while k_cr32_fused / k_cr32_back_all
// wait for it); after the fetch a single 32 x 64 matrix-vector product
// remains.  fetch(xp, xq) puts x_p / x_q (zero where absent) in LDS and ends
// with a barrier; the caller's loads of the tiles are done and synchronised.
// Mp / Mq overwrite Lp / Lq.  Returns x_e in u.
__device__ __forceinline__ d4 mfma32_tn(const double *At, const double *Bt, d4 acc)
{
    // acc (one 16 x 16 block per wave) of A B^T over K = 32, A given
    // transposed (At[t][r]): [r][c] = sum_t At[t][r] Bt[c][t]
    const int w = threadIdx.x >> 6, ra = 16 * (w >> 1), cb = 16 * (w & 1);
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int s = 0; s < 8; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(At[(4 * s + lk) * LP + ra + li],
                                                   Bt[(cb + li) * LP + 4 * s + lk], acc, 0, 0, 0);
    return acc;
}

template <class Fetch>
__device__ __forceinline__ void cr32_back_core(double *Lp, double *Lq, const double *Li,
                                               const double *t, double *z, double *xp,
                                               double *xq, double *u, double (*part)[T32],
                                               bool hp, bool hq, Fetch fetch)
{
    const int tid = threadIdx.x;
    d4 ap = {0.0, 0.0, 0.0, 0.0}, aq = {0.0, 0.0, 0.0, 0.0};
    if (hp) ap = mfma32_tn(Li, Lp, ap);   // Mp[r][c] = sum_t Li[t][r] Lp[c][t]
    if (hq) aq = mfma32_tn(Li, Lq, aq);
    gemv32(Li, t, part, z, true);         // z = L^-T y (ends with a barrier)
    if (hp) put32(Lp, ap, 1.0, false);
    if (hq) put32(Lq, aq, 1.0, false);
    fetch(xp, xq);                        // ends with a barrier
    // x = z - [Mp | Mq] [x_p; x_q]: thread (row r, part of 8 columns)
    const int r = tid & 31, pq = tid >> 5;
    const double *M = pq < 4 ? Lp : Lq;
    const double *v = pq < 4 ? xp : xq;
    const bool on = pq < 4 ? hp : hq;
    const int c0 = 8 * (pq & 3);
    double acc = 0.0;
    if (on) {
#pragma unroll
        for (int c = c0; c < c0 + 8; c++) acc = fma(M[r * LP + c], v[c], acc);
    }
    part[pq][r] = acc;
    __syncthreads();
    if (tid < T32)
        u[tid] = z[tid] - ((((((((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) +
                               part[4][tid]) + part[5][tid]) + part[6][tid]) + part[7][tid]));
    __syncthreads();
}

// back substitution, one launch per level (the no-spin re-solve): x_p and x_q
// come from the previous launches
__global__ __launch_bounds__(256) void k_cr32_back(const int *__restrict__ elim, int nt, int TB,
                                                   long long ld,
                                                   const double *__restrict__ linv,
                                                   const double *__restrict__ crL,
                                                   const double *__restrict__ y,
                                                   double *__restrict__ x)
{
    __shared__ __attribute__((aligned(16))) double Lp[T32 * LP], Lq[T32 * LP], Li[T32 * LP];
    __shared__ __attribute__((aligned(16))) double t[T32], z[T32], xp[T32], xq[T32], u[T32];
    __shared__ double part[8][T32];
    const int tid = threadIdx.x;
    const int e = elim[3 * blockIdx.x], p = elim[3 * blockIdx.x + 1], q = elim[3 * blockIdx.x + 2];
    const long long T2 = (long long)T32 * T32;
    if (p >= 0) load_rm32(crL + T2 * e, Lp);
    if (q >= 0) load_rm32(crL + T2 * (nt + e), Lq);
    load_rm32(linv + T2 * e, Li);
    if (tid < T32) t[tid] = tid < TB ? y[(long long)TB * e + tid] : 0.0;
    __syncthreads();
    cr32_back_core(Lp, Lq, Li, t, z, xp, xq, u, part, p >= 0, q >= 0,
                   [&](double *a, double *b) {
                       if (tid < 2 * T32) {
                           const int nb = tid < T32 ? p : q, i = tid & 31;
                           const long long g = (long long)TB * nb + i;
                           (tid < T32 ? a : b)[i] = (nb >= 0 && i < TB && g < ld) ? x[g] : 0.0;
                       }
                       __syncthreads();
                   });
    if (tid < TB) {
        const long long g = (long long)TB * e + tid;
        if (g < ld) x[g] = u[tid];
    }
}

// ---------------------------------------------------------------------------
// Selected inverse on the camera-aligned CR factors (vlgba_covariance,
// VLGBA_COV_SELECTED): Sigma = S^-1 on the tile-tridiagonal pattern of S, by
// the back substitution's recurrence with matrices in place of vectors.  For a
// record (e, p, q), Li = L_e^-1, Mp = Li^T Lp_e^T, Mq = Li^T Lq_e^T:
//     Sigma_ep = -(Mp Sigma_pp + Mq Sigma_qp)
//     Sigma_eq = -(Mp Sigma_qp^T + Mq Sigma_qq)
//     Sigma_ee = Li^T Li - Sigma_ep Mp^T - Sigma_eq Mq^T
// Levels run last to first, one launch each (p and q were eliminated above e,
// so their tiles come from earlier launches: no in-launch hand-off); one
// workgroup per record.  sig holds three row-major 32 x 32 tiles per CR tile:
// Sigma_ee at sig[e], Xp[e] = Sigma_ep at sig[nt + e], Xq[e] = Sigma_eq at
// sig[2 nt + e].  Sigma_qp is the tile Xq[p] (read as Sigma_pq) or Xp[q]
// (transposed on the way in) of the source tile src[2 x] (chol_selinv_sources;
// src[2 x + 1] = 1: it is p's).  Every sum is an MFMA chain in a fixed order,
// no atomics: a repeated launch gives the same bits.  Sigma_ee is stored
// exactly symmetric (its lower triangle, mirrored).  Padding rows / columns
// (r >= TB, or past ld) carry the identity of the padded factors and never mix
// with real entries, as in the factorisation.
// LDS: seven tiles (Li -> Sigma_ep, Lp -> Mp, Lq -> Mq, Sigma_pp -> Sigma_eq,
// Sigma_qq, Sigma_pq, Li^T -> Sigma_ee), dynamic.
// ---------------------------------------------------------------------------
#define CR32_SELINV_LDS (sizeof(double) * 7 * T32 * LP)

// row-major src[r * 32 + c] -> LDS T[c][r]
__device__ __forceinline__ void load_rm32_t(const double *__restrict__ src, double *T)
{
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = src[(r0 + 8 * u) * T32 + c];
#pragma unroll
    for (int u = 0; u < 4; u++) T[c * LP + r0 + 8 * u] = v[u];
}

// acc (one 16 x 16 block per wave, as mfma32_nt) of A B over K = 32
__device__ __forceinline__ d4 mfma32_nn(const double *A, const double *Bn, d4 acc)
{
    const int w = threadIdx.x >> 6, ra = 16 * (w >> 1), cb = 16 * (w & 1);
    acc = mfma16_nn(A, ra, 0, Bn, 0, cb, acc);
    return mfma16_nn(A, ra, 16, Bn, 16, cb, acc);
}

__global__ __launch_bounds__(256) void k_cr32_selinv(const int *__restrict__ elim,
                                                     const int *__restrict__ src, int nt,
                                                     const double *__restrict__ linv,
                                                     const double *__restrict__ crL,
                                                     double *__restrict__ sig)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int TS = T32 * LP;
    double *Li = sm, *Mp = sm + TS, *Mq = sm + 2 * TS, *Spp = sm + 3 * TS, *Sqq = sm + 4 * TS,
           *Spq = sm + 5 * TS, *See = sm + 6 * TS;
    double *Xp = Li, *Xq = Spp;   // (after their last reads)
    const int x = blockIdx.x;
    const int e = elim[3 * x], p = elim[3 * x + 1], q = elim[3 * x + 2];
    const int st = src[2 * x], sp = src[2 * x + 1];
    const bool hp = p >= 0, hq = q >= 0;
    const long long T2 = (long long)T32 * T32;
    double *See_g = sig + T2 * e, *Xp_g = sig + T2 * (nt + e), *Xq_g = sig + T2 * (2LL * nt + e);
    load_rm32(linv + T2 * e, Li);
    load_rm32_t(linv + T2 * e, See);   // Li^T
    if (hp) {
        load_rm32(crL + T2 * e, Mp);   // Lp_e
        load_rm32(sig + T2 * p, Spp);
    }
    if (hq) {
        load_rm32(crL + T2 * (nt + e), Mq);   // Lq_e
        load_rm32(sig + T2 * q, Sqq);
    }
    if (hp && hq && st >= 0) {   // Sigma_pq: Xq[p], or Xp[q]^T
        if (sp)
            load_rm32(sig + T2 * (2LL * nt + st), Spq);
        else
            load_rm32_t(sig + T2 * (nt + st), Spq);
    }
    __syncthreads();
    const d4 z = {0.0, 0.0, 0.0, 0.0};
    d4 aw = mfma32_tn(Li, See, z);   // W[r][c] = sum_t Li[t][r] Li[t][c]
    d4 ap = z, aq = z;
    if (hp) ap = mfma32_tn(Li, Mp, z);   // Mp[r][c] = sum_t Li[t][r] Lp[c][t]
    if (hq) aq = mfma32_tn(Li, Mq, z);
    __syncthreads();
    if (hp) put32(Mp, ap, 1.0, false);
    if (hq) put32(Mq, aq, 1.0, false);
    __syncthreads();
    // Sigma_ep = -(Mp Sigma_pp + Mq Sigma_pq^T), Sigma_eq = -(Mp Sigma_pq + Mq Sigma_qq)
    // (Sigma_pp, Sigma_qq are exactly symmetric: the nt form reads them as stored)
    ap = aq = z;
    if (hp) ap = mfma32_nt(Mp, Spp, ap);
    if (hp && hq) ap = mfma32_nt(Mq, Spq, ap);
    if (hp && hq) aq = mfma32_nn(Mp, Spq, aq);
    if (hq) aq = mfma32_nt(Mq, Sqq, aq);
    __syncthreads();
    if (hp) put32(Xp, ap, -1.0, false);
    if (hq) put32(Xq, aq, -1.0, false);
    __syncthreads();
    // Sigma_ee = W - Sigma_ep Mp^T - Sigma_eq Mq^T
    d4 as = z;
    if (hp) as = mfma32_nt(Xp, Mp, as);
    if (hq) as = mfma32_nt(Xq, Mq, as);
    put32(See, aw - as, 1.0, false);
    __syncthreads();
    {
        const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + 8 * u;
            See_g[r * T32 + c] = r >= c ? See[r * LP + c] : See[c * LP + r];
        }
    }
    if (hp) store_rm32(Xp_g, Xp);
    if (hq) store_rm32(Xq_g, Xq);
}

// One record of the one-launch back substitution: it loads its three tiles,
// forms z, Mp and Mq (cr32_back_core), then waits for x_p and x_q, which the
// records of the tiles eliminated above it publish as epoch-tagged 8-byte
// granules {epoch, 32-bit half} (write-through agent-scope stores: the data
// is the flag, no fences; MI355X_MICROARCH.md / cdna_hip_programming.md
// Guideline 16, R2).  One wave sweeps one neighbour's 64 granules until every
// tag matches; a spin that never ends sets the timeout word status[1] (the
// host then re-solves the pass with the per-level launches, which never spin)
// instead of hanging.  Same arithmetic as k_cr32_back.
template <bool SC>
__device__ __forceinline__ void cr32_back_body(const cr32_lds &sh, int e, int p, int q, int nt,
                                               int TB, long long ld, const double *linv,
                                               const double *crL, const double *y, double *x,
                                               unsigned long long *xg, unsigned epoch,
                                               double *status)
{
    double *Lp = sh.As, *Lq = sh.Bs, *Li = sh.Cs;
    double *t = sh.rk, *xp = sh.ym, *xq = sh.yp, *u = sh.um, *z = sh.up;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long T2 = (long long)T32 * T32;
    if (p >= 0) load_rm32<SC>(crL + T2 * e, Lp);
    if (q >= 0) load_rm32<SC>(crL + T2 * (nt + e), Lq);
    load_rm32<SC>(linv + T2 * e, Li);
    if (tid < T32) t[tid] = tid < TB ? ldg<SC>(y + (long long)TB * e + tid) : 0.0;
    __syncthreads();
    cr32_back_core(Lp, Lq, Li, t, z, xp, xq, u, sh.part, p >= 0, q >= 0,
                   [&](double *a, double *b) {
                       if (wv < 2) {
                           const int nb = wv == 0 ? p : q;
                           double *dst = wv == 0 ? a : b;
                           if (nb >= 0) {
                               const unsigned long long *g = xg + 64 * (size_t)nb + lane;
                               unsigned long long v = 0;
                               for (unsigned spins = 0;; spins++) {
                                   v = __hip_atomic_load(g, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                                   if (__all((unsigned)(v >> 32) == epoch)) break;
                                   if (spins >= BA_BACK_SPIN_MAX) {
                                       if (lane == 0) status[1] = 1.0;
                                       break;
                                   }
                                   __builtin_amdgcn_s_sleep(2);
                               }
                               // lane 2r: low half of x_r, lane 2r + 1: high half
                               reinterpret_cast<unsigned *>(dst)[lane] = (unsigned)v;
                           } else if (lane < T32) {
                               dst[lane] = 0.0;
                           }
                       }
                       __syncthreads();
                   });
    if (wv == 0) {   // publish x_e: 64 granules, one 8-byte write-through store each
        const unsigned h = reinterpret_cast<const unsigned *>(u)[lane];
        __hip_atomic_store(xg + 64 * (size_t)e + lane, ((unsigned long long)epoch << 32) | h,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < TB) {
        const long long g = (long long)TB * e + tid;
        if (g < ld) x[g] = u[tid];
    }
}

// All levels of the back substitution in ONE launch (the
// 8 level launches were at the launch floor).  Workgroup b takes elimination
// record nrec-1-b (the deepest level first).  Every record's neighbours are
// eliminated at higher levels, so the dependencies form a tree from the top
// level down; the launch is used only when all workgroups are co-resident
// (nrec <= 2 x CUs).
__global__ __launch_bounds__(256) void k_cr32_back_all(const int *__restrict__ elim, int nrec,
                                                       int nt, int TB, long long ld,
                                                       const double *__restrict__ linv,
                                                       const double *__restrict__ crL,
                                                       const double *__restrict__ y,
                                                       double *__restrict__ x,
                                                       unsigned long long *__restrict__ xg,
                                                       unsigned epoch, double *status)
{
    __shared__ __attribute__((aligned(16))) double Lp[T32 * LP], Lq[T32 * LP], Li[T32 * LP];
    __shared__ __attribute__((aligned(16))) double t[T32], xp[T32], xq[T32], u[T32], z[T32];
    __shared__ double part[8][T32];
    const cr32_lds sh{Lp, Lq, Li, nullptr, nullptr, nullptr, t, xp, xq, u, z, part};
    const int rec = nrec - 1 - (int)blockIdx.x;
    const int e = elim[3 * rec], p = elim[3 * rec + 1], q = elim[3 * rec + 2];
    cr32_back_body<false>(sh, e, p, q, nt, TB, ld, linv, crL, y, x, xg, epoch, status);
}

// ---------------------------------------------------------------------------
// The whole camera-aligned cyclic reduction in ONE launch: the level-0
// factor records (3 per eliminated tile), then per level L >= 1 the fused
// records (3 per eliminated tile) and the survivor records, then the back
// substitution records deepest level first -- the schedule and arithmetic of
// k_cr32_factor + k_cr32_level x (nl - 1) + k_cr32_back_all, record for record
// (bit-identical), with the launch boundaries replaced by per-record
// dependencies: a record waits only for the records whose outputs it reads,
//   level L >= 1, tile k (neighbours em / ep eliminated at L-1):
//     role 0 / survivor: roles 0..2 of em and ep at L-1 (L(k, em), L(k, ep),
//     y); roles 1 / 2: only the panels they read (L(k, em) = role 2 of em,
//     L(k, ep) = role 1 of ep, the fill's L(p, em) = role 1 of em or
//     L(q, ep) = role 2 of ep); all: k's own survivor record at L-1 (D_k,
//     r_k) when L >= 2 (survivor records publish D_k and r_k separately: the
//     panel roles wait for D_k only, role 0 for both);
//   survivor at L: L(k, em), L(k, ep) (and D_k at L-1) for D_k, then the
//     neighbours' role 0 (y) and its own r_k at L-1 for r_k;
//   back record of e (eliminated at Le): roles 0..2 of e at Le, then the
//     x granules of its neighbours (as k_cr32_back_all).
// Hand-offs: payload stored sc1 (stg<true>), every storing wave's vmcnt(0),
// a barrier, one lane's sc1 flag store {epoch} per (level, tile, role); the
// consumer's wave 0 polls its <= 7 flags (relaxed agent loads), a barrier,
// then sc1 loads (ldg<true>) of every handed-off byte.  The 96 KB LDS pool
// keeps one workgroup per CU (the row of MI355X_MICROARCH.md's hand-off table
// this protocol follows).  Records wait only on records with lower block
// indices, so in-order dispatch makes progress without co-residency; every
// spin is bounded (timeout word status[1]: the host re-solves with the per-level
// launches).
// ---------------------------------------------------------------------------
// (the block ranges: cr32_fplan, ba_chol_plan.h)

__device__ __forceinline__ void cr32_wait_flags(const unsigned *flag, int nw, const int w[8],
                                                unsigned epoch, double *status)
{
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        int idx = 0;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (lane == q) idx = w[q];
        for (unsigned spins = 0;; spins++) {
            const bool ok = lane >= nw || __hip_atomic_load((const gu32_t *)(flag + idx),
                                                            __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT) == epoch;
            if (__all(ok)) break;
            if (spins >= BA_BACK_SPIN_MAX) {
                if (lane == 0) status[1] = 1.0;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void cr32_publish(unsigned *flag, unsigned epoch, int nflags = 1)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
    __syncthreads();
    if (threadIdx.x < nflags)   // consecutive flag words (role 4: roles 0 and 1)
        __hip_atomic_store((gu32_t *)(flag + threadIdx.x), epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}


// the camera update of a back record's own cameras (ba_dev::camupd_fold)
struct cr32_camupd {
    const double *a;   // nullptr: none
    double *a_new, *rot_new;
    int na, m;
};

// JAC: the folded camera update builds the analytic-Jacobian mode's table
// (rotation_k_jac); everything else is the same code.  (A template of the
// kernel itself, not a body shared by two kernels: with the record pool's
// static LDS declared in a device function the compiler allocated 8 KB more.)
template <bool JAC>
__global__ __launch_bounds__(256) void k_cr32_fused(double *S, long long lds, int TB, long long ld,
                                                    const int *__restrict__ elim,
                                                    const int *__restrict__ frec,
                                                    const int *__restrict__ srec, int nt,
                                                    double *linv, double *crL, double *rhs,
                                                    double *y, double *x, unsigned *flag,
                                                    unsigned long long *xg, unsigned epoch,
                                                    double *status, cr32_fplan P,
                                                    cr32_camupd cu)
{
    CR32_LDS_DECL;
    CR_ST(0);
    const int b = blockIdx.x;
    int L = 0;
    while (L < P.nl && b >= P.b0[L + 1]) L++;
    // flag word of (level, tile, role): 3 = survivor's D_k, 4 = its r_k
    auto fw = [&](int lev, int t, int r) { return 5 * (lev * nt + t) + r; };
    if (L == 0) {
        // three records per tile, or two (roles 0 + 1 merged) when three would
        // not all fit on the CUs at once (one workgroup per CU)
        const int xr = P.l0two ? b / 2 : b / 3;
        const int role = P.l0two ? ((b & 1) ? 2 : 4) : b % 3;
        const int e = elim[3 * xr], p = elim[3 * xr + 1], q = elim[3 * xr + 2];
        CR_ST(1);
        if (!((role == 1 && p < 0) || (role == 2 && q < 0)))
            cr32_factor_body<true>(sh, S, lds, TB, ld, e, p, q, role, nt, linv, crL, rhs, y,
                                   status);
        CR_ST(2);
        if (role == 4)
            cr32_publish(flag + fw(0, e, 0), epoch, 2);
        else
            cr32_publish(flag + fw(0, e, role), epoch);
        CR_ST(3);
        return;
    }
    if (L < P.nl) {
        const int r = b - P.b0[L];
        const int ne = (P.b0[L + 1] - P.b0[L]) - (P.sofs[L + 1] - P.sofs[L]);   // 3 x fused
        int k, p = -1, q = -1, em, ep, role = 3;
        if (r >= ne) {
            const int *sr = srec + 3 * (P.sofs[L] + r - ne);
            k = sr[0];
            em = sr[1];
            ep = sr[2];
        } else {
            const int *fr = frec + 5 * (P.fofs[L] + r / 3);
            role = r % 3;
            k = fr[0];
            p = fr[1];
            q = fr[2];
            em = fr[3];
            ep = fr[4];
        }
        int w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nw = 0;
        if (role == 1 || role == 2) {   // panels only: L(k, em), L(k, ep) and the fill's
            w[nw++] = fw(L - 1, em, 2);  // L(p, em) | L(q, ep) -- not role 0's y / L^-1
            if (role == 1) w[nw++] = fw(L - 1, em, 1);
            if (ep >= 0) {
                w[nw++] = fw(L - 1, ep, 1);
                if (role == 2) w[nw++] = fw(L - 1, ep, 2);
            }
            if (L >= 2) w[nw++] = fw(L - 1, k, 3);
        } else if (role == 3) {         // survivor, D_k first: L(k, em), L(k, ep)
            w[nw++] = fw(L - 1, em, 2);
            if (ep >= 0) w[nw++] = fw(L - 1, ep, 1);
            if (L >= 2) w[nw++] = fw(L - 1, k, 3);
        } else {
            for (int rr = 0; rr < 3; rr++) w[nw++] = fw(L - 1, em, rr);
            if (ep >= 0)
                for (int rr = 0; rr < 3; rr++) w[nw++] = fw(L - 1, ep, rr);
            if (L >= 2) {
                w[nw++] = fw(L - 1, k, 3);
                w[nw++] = fw(L - 1, k, 4);
            }
        }
        // (Tried in round 5: own D_k waited for alone and its loads issued
        // before the neighbours' wait -- 81 -> 86 us: the second poll-and-
        // barrier costs more than the overlapped loads save.)  The flags are
        // polled per operand by the wave that loads it (cr32_level_body's pw),
        // no poll-and-barrier here -- but for a record without a body
        const bool skip = (role == 1 && p < 0) || (role == 2 && q < 0);
        if (skip) cr32_wait_flags(flag, nw, w, epoch, status);
        CR_ST(1);
        // the survivor's r_k: the neighbours' y and its own r_k of level L-1
        auto mid = [&]() {
            cr32_publish(flag + fw(L, k, 3), epoch);
            int w2[8] = {fw(L - 1, em, 0), 0, 0, 0, 0, 0, 0, 0}, n2 = 1;
            if (ep >= 0) w2[n2++] = fw(L - 1, ep, 0);
            if (L >= 2) w2[n2++] = fw(L - 1, k, 4);
            cr32_wait_flags(flag, n2, w2, epoch, status);
        };
        const cr32_pw pw{flag, epoch, status, L, nt};
        if (!skip)
            cr32_level_body<true>(sh, S, lds, TB, ld, k, p, q, em, ep, role, nt, linv, crL, rhs,
                                  y, status, mid, &pw);
        CR_ST(2);
        cr32_publish(flag + fw(L, k, role == 3 ? 4 : role), epoch);
        CR_ST(3);
        return;
    }
    // back substitution, deepest record first
    const int rec = P.nrec - 1 - (b - P.b0[P.nl]);
    int Le = 0;
    while (Le + 1 < P.nl && rec >= P.eofs[Le + 1]) Le++;
    const int e = elim[3 * rec], p = elim[3 * rec + 1], q = elim[3 * rec + 2];
    const int w[8] = {fw(Le, e, 0), fw(Le, e, 1), fw(Le, e, 2), 0, 0, 0, 0, 0};
    cr32_wait_flags(flag, 3, w, epoch, status);
    CR_ST(1);
    // k_camera_update for the tile's own cameras (ba_dev::camupd_fold: x = da in
    // camera order, a tile = TB / na whole cameras), from x_e in LDS: a_new =
    // a + da and the five rotations of its table, lane (camera c, rotation k)
    // of wave 1 -- one Rodrigues chain, on a wave that does not publish the x
    // granules.  The lane's a is loaded ahead of the record's waits; nothing
    // in this launch reads a_new or rot_new.
    const int cl = threadIdx.x & 63, cc0 = cl / 5, ck = cl - 5 * cc0;
    const int cj = (cu.a ? TB / cu.na : 0) * e + cc0;
    const bool con = cu.a && (threadIdx.x >> 6) == 1 && cc0 < TB / cu.na && cj < cu.m;
    double av[10];   // (na <= 10: the Euclidean models)
    if (con) {
#pragma unroll
        for (int cc = 0; cc < 10; cc++)
            av[cc] = cc < cu.na ? cu.a[(size_t)cu.na * cj + cc] : 0.0;
    }
    cr32_back_body<true>(sh, e, p, q, nt, TB, ld, linv, crL, y, x, xg, epoch, status);
    CR_ST(2);
    if (con) {
#pragma unroll
        for (int cc = 0; cc < 10; cc++) {
            if (cc < cu.na) {
                av[cc] = av[cc] + sh.um[cu.na * cc0 + cc];
                if (ck == 0) cu.a_new[(size_t)cu.na * cj + cc] = av[cc];
            }
        }
        if constexpr (JAC)
            rotation_k_jac(av, ck, cu.rot_new + 45 * (size_t)cj);
        else
            rotation_k(av, ck, cu.rot_new + 45 * (size_t)cj);
    }
    CR_ST(3);
}

__global__ __launch_bounds__(256) void k_cr_back(const int *__restrict__ elim, int nt,
                                                 const double *__restrict__ linv,
                                                 const double *__restrict__ crL,
                                                 const double *__restrict__ y,
                                                 double *__restrict__ x)
{
    __shared__ double Ls[NB * LP];
    __shared__ double t[NB], u[NB];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x;
    const int e = elim[3 * blockIdx.x], p = elim[3 * blockIdx.x + 1], q = elim[3 * blockIdx.x + 2];
    const long long T2 = (long long)NB * NB;
    if (tid < NB) t[tid] = y[(long long)NB * e + tid];
    if (p >= 0) {
        load_rowmajor(crL + T2 * e, Ls);
        if (tid < NB) u[tid] = x[(long long)NB * p + tid];
        __syncthreads();
        gemv64_t(Ls, u, part, u, 1.0);
        if (tid < NB) t[tid] -= u[tid];
        __syncthreads();
    }
    if (q >= 0) {
        load_rowmajor(crL + T2 * (nt + e), Ls);
        if (tid < NB) u[tid] = x[(long long)NB * q + tid];
        __syncthreads();
        gemv64_t(Ls, u, part, u, 1.0);
        if (tid < NB) t[tid] -= u[tid];
        __syncthreads();
    }
    load_rowmajor(linv + T2 * e, Ls);
    __syncthreads();
    gemv64_t(Ls, t, part, x + (long long)NB * e, 1.0);
}

// ---------------------------------------------------------------------------
// One launch builds every envelope tile of S for the factorisation: zeros
// (clearing the previous factorisation's in-place results and fill), the
// lower entries of the co-visible blocks that overlap the tile (S_jk, row >=
// col; bundle_euclid.m:192-193), and for diagonal tiles the pinv rule for
// exactly-zero rows (App. A Q2, Q8: unit diagonal, rhs 0; padding rows past
// NA*m included).  Workgroup 0 also clears the factorisation status.
// Replaces k_zero_env + k_assemble + k_fix_diag + two memsets (5 launches).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assemble_tiles(
    double *__restrict__ S, long long lds, const int *__restrict__ env,
    const int *__restrict__ tb_ptr, const int *__restrict__ tb_blk,
    const int *__restrict__ blk_jk, const double *__restrict__ sblk, int na, long long ld,
    double *__restrict__ rhs, double *__restrict__ status, const int *__restrict__ crow,
    const int *__restrict__ rowsrc, const double *__restrict__ rhs_src)
{
    __shared__ double T[NB * (NB + 1)];
    const int ti = env[2 * blockIdx.x], tk = env[2 * blockIdx.x + 1], tid = threadIdx.x;
    for (int q = tid; q < NB * (NB + 1); q += 256) T[q] = 0.0;
    if (blockIdx.x == 0 && tid == 0) {
        status[0] = 0.0;   // non-positive pivot
        status[1] = 0.0;   // bounded hand-off spin gave up
    }
    __syncthreads();
    const long long r0 = (long long)NB * ti, c0 = (long long)NB * tk;
    const int na2 = na * na;
    const int u0 = tb_ptr[blockIdx.x], nq = (tb_ptr[blockIdx.x + 1] - u0) * na2;
    // (block, entry) pairs, all lanes busy; four a lane per step with their
    // three dependent loads (block id, its cameras, the entry) in flight
    // together -- each item writes its own tile entry, so the same tile
    for (int q0 = tid; q0 < nq; q0 += 4 * 256) {
        int lq[4], bq[4], jq[4], kq[4];
        double vq[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int q = min(q0 + 256 * t, nq - 1), u = q / na2;
            lq[t] = q - na2 * u;
            bq[t] = tb_blk[u0 + u];
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            jq[t] = blk_jk[2 * bq[t]];
            kq[t] = blk_jk[2 * bq[t] + 1];
            vq[t] = sblk[(size_t)na2 * bq[t] + lq[t]];
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
        if (q0 + 256 * t >= nq) break;
        const int l = lq[t], bj = jq[t], bc = kq[t];
        const int r = l % na, c = l / na;
        long long row, col;
        if (!crow) {
            row = (long long)na * bj + r;
            col = (long long)na * bc + c;
        } else {   // nested-dissection rows: S_kj = S_jk^T where camera k's rows come later
            row = crow[bj] + r;
            col = crow[bc] + c;
            if (row < col && bj != bc) {
                const long long t = row;
                row = col;
                col = t;
            }
        }
        if (row < col || row < r0 || row >= r0 + NB || col < c0 || col >= c0 + NB) continue;
        T[(row - r0) * (NB + 1) + (col - c0)] = vq[t];
        }
    }
    __syncthreads();
    if (ti == tk && tid < NB) {   // pinv semantics for exactly-zero rows, padding rows
        double *d = T + tid * (NB + 1) + tid;
        const long long r = r0 + tid;
        if (rowsrc) {   // gather the row-ordered rhs (nested dissection)
            const int src = rowsrc[r];
            rhs[r] = src >= 0 ? rhs_src[src] : 0.0;
        }
        if (*d == 0.0) {
            *d = 1.0;
            rhs[r] = 0.0;
        } else if (r >= ld) {
            rhs[r] = 0.0;
        }
    }
    __syncthreads();
    double *base = S + r0 + lds * c0;
    const int r = tid & 63, cq = tid >> 6;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int c = cq + 4 * u;
        base[r + lds * c] = T[r * (NB + 1) + c];
    }
}

// zero every envelope tile of S (fill from the previous factorisation)
__global__ void k_zero_env(double *__restrict__ S, long long lds, const int *__restrict__ env)
{
    const int i = env[2 * blockIdx.x], k = env[2 * blockIdx.x + 1];
    double *base = S + (long long)NB * i + lds * (long long)NB * k;
    for (int q = threadIdx.x; q < NB * NB; q += blockDim.x) {
        const int r = q & (NB - 1), c = q >> 6;
        base[r + lds * c] = 0.0;
    }
}

// pinv semantics for exactly-zero rows (App. A Q2, Q8): such a row/column of
// S is exactly zero (its A columns are zero, hence its W and Y rows); give it
// a unit diagonal and a zero right-hand side so da = 0 there.
__global__ void k_fix_diag(double *__restrict__ S, double *__restrict__ rhs, long long lds)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= lds) return;
    double *d = S + r + lds * r;
    if (*d == 0.0) {
        *d = 1.0;
        rhs[r] = 0.0;
    }
}

// ---------------------------------------------------------------------------
// Sequential reduced solve (dense_solve = 3, the parity mode): left-looking
// Cholesky of the lower triangle, every sum in ascending index order, then the
// two triangular solves -- exactly the loops of the CPU oracle's
// sequential Cholesky, so da is bit-identical to it.  One
// workgroup: the diagonal entry of column j by lane 0, the column's rows by
// the other lanes (each row's sum stays sequential).  The exactly-zero rows
// have their unit diagonal / zero rhs from k_assemble_tiles (App. A Q8).
// For the small problems of the parity tests (ld of a few hundred).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chol_seq(double *__restrict__ S, long long lds,
                                                  int n, double *__restrict__ rhs,
                                                  double *__restrict__ x,
                                                  double *__restrict__ status)
{
    __shared__ double piv;
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (tid == 0) {
            double s = S[j + lds * j];
            for (int k = 0; k < j; k++) {
                const double l = S[j + lds * k];
                s = s - l * l;
            }
            if (!(s > 0.0)) bad = 1;
            piv = sqrt(s);
            S[j + lds * j] = piv;
        }
        __syncthreads();
        if (bad) break;
        const double p = piv;
        for (int i = j + 1 + tid; i < n; i += 256) {
            double t = S[i + lds * j];
            for (int k = 0; k < j; k++) t = t - S[i + lds * k] * S[j + lds * k];
            S[i + lds * j] = t / p;
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) status[0] = 1.0;
        return;
    }
    if (tid == 0) {   // L y = rhs, then L^T x = y (x over y in place)
        for (int i = 0; i < n; i++) {
            double t = rhs[i];
            for (int k = 0; k < i; k++) t = t - S[i + lds * k] * x[k];
            x[i] = t / S[i + lds * i];
        }
        for (int i = n - 1; i >= 0; i--) {
            double t = x[i];
            for (int k = i + 1; k < n; k++) t = t - S[k + lds * i] * x[k];
            x[i] = t / S[i + lds * i];
        }
    }
}

// ---------------------------------------------------------------------------
// pinv(S) e_ from the symmetric eigen-decomposition (the fallback when the
// Cholesky meets a non-positive pivot: bundle_euclid.m:193 always takes
// pinv(S)*e_).  MATLAB's pinv keeps the singular values
// (= |eigenvalues| here) above max(size) * eps(max singular value).
//   k_pinv_w: w_k = (v_k . rhs) / ev_k  for |ev_k| > tol, else 0
//   k_pinv_x: da_i = sum_k V[i][k] w_k
// one workgroup per output entry, fixed-order reductions (deterministic).
// ---------------------------------------------------------------------------
static __device__ double dev_eps_of(double x)
{
    if (!(x > 0.0)) return 4.9406564584124654e-324;
    int e;
    (void)frexp(x, &e);
    return ldexp(1.0, e - 53);
}

__global__ __launch_bounds__(256) void k_pinv_w(const double *__restrict__ V,
                                                const double *__restrict__ ev, long long ld,
                                                const double *__restrict__ rhs,
                                                double *__restrict__ w)
{
    __shared__ double red[256];
    const long long k = blockIdx.x;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < ld; i += 256) acc += V[i + ld * k] * rhs[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double emax = fmax(fabs(ev[0]), fabs(ev[ld - 1]));
        const double tol = (double)ld * dev_eps_of(emax);
        w[k] = fabs(ev[k]) > tol ? red[0] / ev[k] : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_pinv_x(const double *__restrict__ V, long long ld,
                                                const double *__restrict__ w,
                                                double *__restrict__ da)
{
    __shared__ double red[256];
    const long long i = blockIdx.x;
    double acc = 0.0;
    for (long long k = threadIdx.x; k < ld; k += 256) acc += V[i + ld * k] * w[k];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) da[i] = red[0];
}

int ba_pinv_apply(ba_dev *d, const double *V, const double *ev, long long ld, const double *rhs,
                  double *work, double *da)
{
    if (ld <= 0) return 0;
    k_pinv_w<<<(unsigned)ld, 256, 0, d->stream>>>(V, ev, ld, rhs, work);
    k_pinv_x<<<(unsigned)ld, 256, 0, d->stream>>>(V, ld, work, da);
    return -(int)hipGetLastError();
}

// ===========================================================================
// (counted in c->bytes: vlgba_plan_info [32])
template <typename T>
static int dev_alloc(ba_chol *c, T **p, size_t bytes)
{
    *p = (T *)ba_dmalloc(bytes);
    if (!*p) return -(int)hipErrorOutOfMemory;
    c->bytes += (long long)bytes;
    return 0;
}

// ---- the solve's setup: plan on the host (ba_chol_plan.cpp), allocate, upload
static bool env_is(const char *name, char c)
{
    const char *e = std::getenv(name);
    return e && e[0] == c;
}

int ba_chol_setup(ba_dev *d, const int *blk_jk, int nb)
{
    const chol_plan_opts opt = {!env_is("VLGBA_CR_FUSED", '0'), env_is("VLGBA_ND", '0'),
                                env_is("VLGBA_ND", 'v'), !env_is("VLGBA_ND_GROUPED", '0'),
                                env_is("VLGBA_ENV_RUNNER", '1')};
    const chol_plan_in in = {d->m, d->na, d->ld, d->lds, d->ncu, d->dense_solve, blk_jk, nb, opt};
    ba_chol *c = d->chol = new ba_chol();   // (zeroed: null pointers, epochs 0)
    const chol_plan &P = c->plan;
    TRY_RC(chol_plan_build(in, c->plan));
    c->env_runner = P.env_runner;

    const int nt = P.nt;
    auto put = [&](int *dst, const std::vector<int> &v) -> int {   // (nothing when empty)
        if (!v.empty())
            VLGBA_CHECK(hipMemcpyAsync(dst, v.data(), sizeof(int) * v.size(),
                                       hipMemcpyHostToDevice, d->stream));
        return 0;
    };
    if (P.cr_nlev > 0) {   // cyclic reduction: its records, L(p, e) | L(q, e)
        const int ntc = P.cr_tiles();
        if (P.cr32) {
            TRY_RC(dev_alloc(c, &c->xgran, sizeof(unsigned long long) * 64 * (size_t)ntc));
            VLGBA_CHECK(hipMemsetAsync(c->xgran, 0, sizeof(unsigned long long) * 64 * (size_t)ntc,
                                       d->stream));
            if (P.cr_fused) {
                const size_t nfl = (size_t)5 * P.cr_nlev * ntc;
                TRY_RC(dev_alloc(c, &c->crflag, sizeof(unsigned) * nfl));
                VLGBA_CHECK(hipMemsetAsync(c->crflag, 0, sizeof(unsigned) * nfl, d->stream));
            }
            TRY_RC(dev_alloc(c, &c->crf, sizeof(int) * (P.frec.size() + 1)));
            TRY_RC(dev_alloc(c, &c->crs, sizeof(int) * (P.srec.size() + 1)));
            TRY_RC(put(c->crf, P.frec));
            TRY_RC(put(c->crs, P.srec));
            VLGBA_CHECK(hipStreamSynchronize(d->stream));
        }
        TRY_RC(dev_alloc(c, &c->cr_elim, sizeof(int) * P.elim.size()));
        TRY_RC(dev_alloc(c, &c->cr_keep, sizeof(int) * (P.keep.size() + 1)));
        TRY_RC(dev_alloc(c, &c->crL, sizeof(double) * 2 * (size_t)ntc *
                                      (P.cr32 ? T32 * T32 : NB * NB)));
        TRY_RC(put(c->cr_elim, P.elim));
        TRY_RC(put(c->cr_keep, P.keep));
    }
    // per envelope tile: the co-visible blocks (j >= k) overlapping it
    TRY_RC(dev_alloc(c, &c->tb_ptr, sizeof(int) * P.tptr.size()));
    TRY_RC(dev_alloc(c, &c->tb_blk, sizeof(int) * (P.tblk.size() + 1)));
    TRY_RC(put(c->tb_ptr, P.tptr));
    TRY_RC(put(c->tb_blk, P.tblk));
    VLGBA_CHECK(hipStreamSynchronize(d->stream));
    // the factor's storage: S (dense, column major), the diagonal tiles'
    // inverses, the forward-solve result (+ the 32-row CR's last tile)
    const bool nd = P.nd_np > 0;
    const long long sdim = nd ? P.slds : d->lds;
    TRY_RC(dev_alloc(c, &c->S, sizeof(double) * (size_t)(sdim * sdim)));
    TRY_RC(dev_alloc(c, &c->linv, sizeof(double) * (size_t)(sdim / NB) * NB * NB));
    TRY_RC(dev_alloc(c, &c->ywork, sizeof(double) * (size_t)(sdim + NB)));
    if (nd) {
        auto up = [&](int **dst, const std::vector<int> &v) -> int {
            TRY_RC(dev_alloc(c, dst, sizeof(int) * (v.size() + 1)));
            return put(*dst, v);
        };
        TRY_RC(up(&c->nd_crow, P.crow));
        TRY_RC(up(&c->nd_prow, P.prow));
        TRY_RC(up(&c->nd_rowsrc, P.rowsrc));
        TRY_RC(up(&c->nd_pair, P.pairs));
        TRY_RC(up(&c->nd_pptr, P.pptr));
        TRY_RC(up(&c->nd_rec, P.rec));
        TRY_RC(up(&c->nd_klist, P.klist));
        TRY_RC(dev_alloc(c, &c->nd_rhs, sizeof(double) * (size_t)P.slds));
        TRY_RC(dev_alloc(c, &c->nd_x, sizeof(double) * (size_t)P.slds));
        TRY_RC(dev_alloc(c, &c->nd_part, sizeof(double) * ((size_t)P.nd_nrec + 1) * (NB * NB + NB)));
        VLGBA_CHECK(hipStreamSynchronize(d->stream));
    }
    TRY_RC(dev_alloc(c, &c->pan_list, sizeof(int) * (P.pan_list.size() + 1)));
    if (P.back_one_launch) {
        TRY_RC(dev_alloc(c, &c->pan_ptr, sizeof(int) * (nt + 1)));
        TRY_RC(put(c->pan_ptr, P.pan_ptr));
        TRY_RC(dev_alloc(c, &c->xgran64, sizeof(unsigned long long) * 128 * (size_t)nt));
        VLGBA_CHECK(hipMemsetAsync(c->xgran64, 0, sizeof(unsigned long long) * 128 * (size_t)nt,
                                   d->stream));
    }
    if (P.handoff) {   // the factor's in-launch hand-off
        TRY_RC(dev_alloc(c, &c->kflag, sizeof(unsigned) * (size_t)nt));
        VLGBA_CHECK(hipMemsetAsync(c->kflag, 0, sizeof(unsigned) * (size_t)nt, d->stream));
        // runner mode's flags: lflag | dflag | uflag | pflag, nt each, then
        // the runner's timeout word.  Opt-in (VLGBA_ENV_RUNNER=1): the runner
        // makes progress only while its stream has a hardware queue of its own
        if (P.runner_flags) {
            const size_t nw = 4 * (size_t)nt + 1;
            TRY_RC(dev_alloc(c, &c->rflag, sizeof(unsigned) * nw));
            VLGBA_CHECK(hipMemsetAsync(c->rflag, 0, sizeof(unsigned) * nw, d->stream));
        }
    }
    TRY_RC(dev_alloc(c, &c->env_tiles, sizeof(int) * (P.env.size() + 1)));
    TRY_RC(put(c->pan_list, P.pan_list));
    VLGBA_CHECK(hipMemcpyAsync(c->env_tiles, P.env.data(), sizeof(int) * P.env.size(),
                               hipMemcpyHostToDevice, d->stream));
    VLGBA_CHECK(hipMemsetAsync(c->S, 0, sizeof(double) * sdim * sdim, d->stream));
    VLGBA_CHECK(hipStreamSynchronize(d->stream));
    return 0;
}

// also after a setup that returned early (every device pointer of *d->chol is
// null or owned) and for a context that was never set up (stage mode:
// d->chol is null).  The runner's stream is the process's (env_runner_stream)
void ba_chol_free(ba_dev *d)
{
    ba_chol *c = d->chol;
    if (!c) return;
    void *dev[] = {c->S,       c->linv,     c->ywork,  c->nd_crow, c->nd_prow, c->nd_rowsrc,
                   c->nd_rhs,  c->nd_x,     c->nd_pair, c->nd_pptr, c->nd_rec, c->nd_klist,
                   c->nd_part, c->xgran,    c->rflag,  c->crflag,  c->crf,     c->crs,
                   c->cr_elim, c->cr_keep,  c->crL,    c->tb_ptr,  c->tb_blk,  c->pan_list,
                   c->pan_ptr, c->xgran64,  c->kflag,  c->env_tiles};
    for (void *q : dev)
        if (q) ba_dfree(q);
    delete c;
    d->chol = nullptr;
}

int ba_assemble_tiles(ba_dev *d)
{
    if (d->asm_direct) return 0;   // k_schur_reduce wrote S (and reset the status)
    const ba_chol *c = d->chol;
    const bool nd = c->plan.nd_np > 0;
    const long long slds = c->plan.slds;
    k_assemble_tiles<<<c->plan.n_env(), 256, 0, d->stream>>>(
        c->S, nd ? slds : d->lds, c->env_tiles, c->tb_ptr, c->tb_blk, d->blk_jk, d->sblk, d->na,
        nd ? slds : d->ld, nd ? c->nd_rhs : d->rhs, d->scal + 4, nd ? c->nd_crow : nullptr,
        nd ? c->nd_rowsrc : nullptr, d->rhs);
    return -(int)hipGetLastError();
}

int ba_chol_prepare(ba_dev *d)
{
    const ba_chol *c = d->chol;
    k_zero_env<<<c->plan.n_env(), 256, 0, d->stream>>>(c->S, d->lds, c->env_tiles);
    return -(int)hipGetLastError();
}

// the same rule on a dense ld x ld S (the natural-order retry of a
// nested-dissection pivot, ba_solver.cpp) and the camera-order rhs
int ba_fix_diag_plain(ba_dev *d, double *S, long long ld)
{
    k_fix_diag<<<(int)((ld + 255) / 256), 256, 0, d->stream>>>(S, d->rhs, ld);
    return -(int)hipGetLastError();
}

int ba_chol_fix_diag(ba_dev *d)
{
    k_fix_diag<<<(int)((d->lds + 255) / 256), 256, 0, d->stream>>>(d->chol->S, d->rhs,
                                                                    d->lds);
    return -(int)hipGetLastError();
}

// runner mode (k_env_runner) for this factorization?  Needs the hand-off, the
// device panel pointers and the flags; off under per-kernel timing (one stream)
// and, for the rest of this context, after one of the runner's own hand-offs
// gave up (ba_env_runner_timed_out): the runner needs its side stream on a
// hardware queue of its own (with the library stream's column launches queued
// behind it on a shared queue every wait times out)
int ba_env_runner_timed_out(ba_dev *d)
{
    ba_chol *c = d->chol;   // (a solving context: never null here)
    if (!c->env_runner || !c->rflag) return 0;
    unsigned *rto = c->rflag + 4 * (size_t)c->plan.nt;
    unsigned h = 0;
    if (hipMemcpyAsync(&h, rto, sizeof h, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess)
        return -1;
    if (!h) return 0;
    c->env_runner = 0;
    std::fprintf(stderr, "[vlgba] envelope runner off for this context: one of its hand-offs "
                         "timed out (its stream shares a hardware queue?)\n");
    return 1;
}

// runs shorter than VLGBA_ENV_RUNNER_MIN columns (default 8) keep the column
// launches alone: the fork / join of the runner's stream (two cross-stream
// event waits a factorization) outweighs a few columns' savings (~3-5 us each)
static int env_run_min()
{
    const char *e = std::getenv("VLGBA_ENV_RUNNER_MIN");
    return e ? std::max(1, std::atoi(e)) : 8;
}

// the runner's stream: one per device for the process, at the highest
// priority, made on first use (a stream per context cost ~1 ms a context in
// the growing replay).  Two contexts factoring on one device at once
// serialise their runners; the later one's hand-offs may then give up (the
// re-solve path) -- correct, only slower.
static hipStream_t env_runner_stream()
{
    static std::mutex mu;
    static hipStream_t st[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!st[dev]) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&st[dev], hipStreamNonBlocking, hi) != hipSuccess)
            st[dev] = nullptr;
    }
    return st[dev];
}

static bool env_run_on(ba_dev *d, const unsigned *kflag, int ncols)
{
    ba_chol *c = d->chol;
    if (!(c->env_runner && kflag && c->pan_ptr && c->rflag && !(d->kt && d->kt->on) &&
          ncols >= env_run_min()))
        return false;
    if (!c->rstream) c->rstream = env_runner_stream();
    if (!c->rstream) {
        c->env_runner = 0;
        return false;
    }
    return true;
}

static env_rm env_rm_of(const ba_dev *d, int kend)
{
    unsigned *rflag = d->chol->rflag;
    const size_t nt = (size_t)d->chol->plan.nt;
    if (!rflag) return env_rm{};
    return env_rm{rflag, rflag + nt, rflag + 2 * nt, rflag + 3 * nt, rflag + 4 * nt, kend};
}

// fork the side stream off the library stream and start the runner there.
// Nonzero: nothing was launched (the caller runs the column launches alone)
// or the launch failed (the error is returned).
static int env_runner_start(ba_dev *d, const env_runs &Rn, long long L, double *rhs)
{
    ba_chol *c = d->chol;
    if (c->debug_runner_fail > 0) {   // vlgba_debug_force_status word 6
        c->debug_runner_fail--;
        return -(int)hipErrorLaunchFailure;
    }
    const size_t smem4 = sizeof(double) * 4 * NB * LP;
    TRY_RC(ba_ensure_dyn_lds((const void *)k_env_runner, smem4));
    VLGBA_CHECK(hipEventRecord(d->ev_fork, d->stream));
    VLGBA_CHECK(hipStreamWaitEvent(c->rstream, d->ev_fork, 0));
    k_env_runner<<<Rn.np, 256, smem4, c->rstream>>>(c->S, L, c->pan_ptr, c->pan_list, Rn,
                                                    c->linv, rhs, c->ywork, d->scal + 4,
                                                    c->kflag, env_rm_of(d, 0), c->fac_epoch);
    TRY_RC(-(int)hipGetLastError());
    VLGBA_CHECK(hipEventRecord(d->ev_join, c->rstream));
    c->runner_runs++;
    return 0;
}

// the envelope's tile columns k0 .. k1-1 (k_factor_step), column k0 taking no
// pending update of column k0-1.  A runner that does not start leaves the
// columns to the launches alone (the same factorization, bit for bit).
static int envelope_columns(ba_dev *d, int k0, int k1, long long L, double *rhs,
                            unsigned *kflag)
{
    ba_chol *c = d->chol;
    // two LDS tiles with the hand-off (two workgroups per CU), three without
    const size_t smem3 = sizeof(double) * 3 * NB * LP, smem2 = sizeof(double) * 2 * NB * LP;
    bool run = k1 > k0 && env_run_on(d, kflag, k1 - k0);
    if (run) {
        env_runs Rn{};
        Rn.np = 1;
        Rn.k0[0] = k0;
        Rn.k1[0] = k1;
        if (env_runner_start(d, Rn, L, rhs)) run = false;
    }
    const std::vector<int> &pan_ptr = c->plan.pan_ptr, &pan_list = c->plan.pan_list;
    for (int k = k0; k < k1; k++) {
        const int p0 = pan_ptr[k], T = pan_ptr[k + 1] - p0;
        const int q0 = k > k0 ? pan_ptr[k - 1] : 0, Tp = k > k0 ? p0 - q0 : 0;
        // column k-1's trailing pairs below row k (see k_factor_step)
        const int kin = Tp > 0 && pan_list[q0] == k;
        const int Tr = Tp - kin, ntr = Tr * (Tr + 1) / 2;
        const int nw = ntr;   // one workgroup per trailing pair
        KT_B(d);
        k_factor_step<<<1 + T + nw, 256, kflag ? smem2 : smem3, d->stream>>>(
            c->S, L, k, c->pan_list + p0, T, c->pan_list + q0, Tp, c->linv, rhs, c->ywork,
            d->scal + 4, kflag, c->fac_epoch, ntr, nw, env_rm_of(d, run ? k1 : 0));
        KT_E(d, KT_FACTOR);
    }
    if (run) VLGBA_CHECK(hipStreamWaitEvent(d->stream, d->ev_join, 0));
    return -(int)hipGetLastError();
}

// x = L^-T y of the envelope factor (ywork holds y; consumed)
static int envelope_backward(ba_dev *d, long long L, double *x, int nospin)
{
    ba_chol *c = d->chol;
    const int nt = c->plan.nt;
    if (c->xgran64 && !nospin) {   // every column co-resident: the backward solve in one launch
        if (++c->back_epoch == 0) c->back_epoch = 1;
        const size_t smem2 = sizeof(double) * 2 * NB * LP;
        TRY_RC(ba_ensure_dyn_lds((const void *)k_backward_all, smem2));
        KT_B(d);
        k_backward_all<<<nt, 256, smem2, d->stream>>>(c->S, L, nt, c->pan_ptr, c->pan_list,
                                                       c->linv, c->ywork, x, c->xgran64,
                                                       c->back_epoch, d->scal + 4);
        KT_E(d, KT_BACKWARD);
        return -(int)hipGetLastError();
    }
    for (int k = nt - 1; k >= 0; k--) {
        const int j0 = c->plan.tfirst[k];
        KT_B(d);
        k_backward<<<k - j0 + 1, 256, 0, d->stream>>>(c->S, L, k, j0, c->linv, c->ywork, x);
        KT_E(d, KT_BACKWARD);
    }
    return -(int)hipGetLastError();
}

// The factor half of the camera-aligned CR, one launch per level: L_e^-1 into
// linv, the panels into crL, y into ywork, the pivot status into scal[4]
// (ba_chol_solve's per-level path, and the selected inverse of
// vlgba_covariance, which runs no back substitution after it)
int ba_cr32_factor(ba_dev *d)
{
    ba_chol *c = d->chol;
    const std::vector<int> &eptr = c->plan.eptr;
    const std::vector<int> &fptr = c->plan.fptr, &sptr = c->plan.sptr;
    const int ncu32 = d->ncu;
    const int n32 = c->plan.nt32, TB = c->plan.tb32;
    {   // level 0 on the assembled S
        const int ne = eptr[1];
        const int fs = 3 * ne <= 2 * ncu32;   // ~60 KB LDS: two workgroups per CU
        KT_B(d);
        k_cr32_factor<<<fs ? 3 * ne : ne, 256, 0, d->stream>>>(
            c->S, d->lds, TB, d->ld, c->cr_elim, n32, c->linv, c->crL, d->rhs, c->ywork,
            d->scal + 4, fs);
        KT_E(d, KT_CR_FACTOR);
    }
    // levels >= 1: the previous level's update folded into the factor launch
    for (int l = 1; l < c->plan.cr_nlev; l++) {
        const int f0 = fptr[l], ne = fptr[l + 1] - f0;
        const int s0 = sptr[l], ns = sptr[l + 1] - s0;
        KT_B(d);
        k_cr32_level<<<3 * ne + ns, 256, 0, d->stream>>>(
            c->S, d->lds, TB, d->ld, c->crf + 5 * f0, ne, c->crs + 3 * s0, n32, c->linv,
            c->crL, d->rhs, c->ywork, d->scal + 4);
        KT_E(d, KT_CR_FACTOR);
    }
    return -(int)hipGetLastError();
}

// The selected inverse's descent on the factors ba_cr32_factor left: levels
// last to first, one launch each.  sig: [3][nt32][32 * 32] doubles; src: device
// [2 * records] (chol_selinv_sources, the source record replaced by its tile)
int ba_cr32_selinv(ba_dev *d, const int *src, double *sig)
{
    ba_chol *c = d->chol;
    const std::vector<int> &eptr = c->plan.eptr;
    TRY_RC(ba_ensure_dyn_lds((const void *)k_cr32_selinv, CR32_SELINV_LDS));
    for (int l = c->plan.cr_nlev - 1; l >= 0; l--) {
        const int e0 = eptr[l], ne = eptr[l + 1] - e0;
        k_cr32_selinv<<<ne, 256, CR32_SELINV_LDS, d->stream>>>(
            c->cr_elim + 3 * e0, src + 2 * e0, c->plan.nt32, c->linv, c->crL, sig);
    }
    return -(int)hipGetLastError();
}

// host: per elimination record the tile holding Sigma_qp (-1: none) and whether
// it is p's, for ba_cr32_selinv: src [2 * nt32] (one record per tile)
int ba_cr32_selinv_sources(const ba_dev *d, int *src)
{
    const ba_chol *c = d->chol;
    if (!c || !(c->plan.cr_nlev > 0 && c->plan.cr32)) return -1000;
    const std::vector<int> &elim = c->plan.elim;
    std::vector<int> s;
    if (chol_selinv_sources(elim, c->plan.eptr, s) || s.size() != 2 * (size_t)c->plan.nt32)
        return -1000;
    for (size_t i = 0; i < s.size(); i += 2) {
        src[i] = s[i] >= 0 ? elim[3 * (size_t)s[i]] : -1;
        src[i + 1] = s[i + 1];
    }
    return 0;
}

// the whole CR in one launch (JAC: the table its folded camera update builds)
template <bool JAC>
static void launch_cr32_fused(ba_dev *d, const cr32_fplan &P, const cr32_camupd &cu)
{
    ba_chol *c = d->chol;
    k_cr32_fused<JAC><<<P.b0[P.nl] + P.nrec, 256, 0, d->stream>>>(
        c->S, d->lds, c->plan.tb32, d->ld, c->cr_elim, c->crf, c->crs, c->plan.nt32, c->linv,
        c->crL, d->rhs, c->ywork, d->da, c->crflag, c->xgran, c->back_epoch, d->scal + 4, P, cu);
}

int ba_chol_solve(ba_dev *d, bool *cam_updated, int nospin)
{
    ba_chol *c = d->chol;
    const chol_plan &pl = c->plan;
    const int nt = pl.nt;
    *cam_updated = false;   // only the one-launch CR below does the camera update
    const size_t smem3 = sizeof(double) * 3 * NB * LP;
    const std::vector<int> &eptr = pl.eptr, &kptr = pl.kptr;
    TRY_RC(ba_ensure_dyn_lds((const void *)k_factor_step, smem3));
    TRY_RC(ba_ensure_dyn_lds((const void *)k_cr_factor, smem3));
    TRY_RC(ba_ensure_dyn_lds((const void *)k_cr_update, smem3));
    if (d->dense_solve == 3) {   // sequential parity solve
        KT_B(d);
        k_chol_seq<<<1, 256, 0, d->stream>>>(c->S, d->lds, (int)d->ld, d->rhs, d->da,
                                             d->scal + 4);
        KT_E(d, KT_FACTOR);
        return -(int)hipGetLastError();
    }
    if (pl.cr_nlev > 0 && pl.cr32 && pl.cr_fused && c->crflag && !nospin) {   // one launch
        const cr32_fplan &P = pl.fplan;
        if (++c->back_epoch == 0) c->back_epoch = 1;
        cr32_camupd cu{};
        if (d->camupd_fold) {   // the next update launches no k_camera_update
            cu = cr32_camupd{d->a, d->a_new, d->rot_new, d->na, d->m};
            *cam_updated = true;
        }
        KT_B(d);
        if (d->jac) launch_cr32_fused<true>(d, P, cu);
        else launch_cr32_fused<false>(d, P, cu);
        KT_E(d, KT_CR_FACTOR);
        return -(int)hipGetLastError();
    }
    if (pl.cr_nlev > 0 && pl.cr32) {   // camera-aligned 32-row tiles
        const int n32 = pl.nt32, TB = pl.tb32;
        TRY_RC(ba_cr32_factor(d));
        const int nrec = eptr[pl.cr_nlev];
        if (c->xgran && nrec <= 2 * d->ncu && !nospin) {   // every record co-resident: one launch
            if (++c->back_epoch == 0) c->back_epoch = 1;
            KT_B(d);
            k_cr32_back_all<<<nrec, 256, 0, d->stream>>>(c->cr_elim, nrec, n32, TB, d->ld,
                                                         c->linv, c->crL, c->ywork, d->da,
                                                         c->xgran, c->back_epoch, d->scal + 4);
            KT_E(d, KT_CR_BACK);
            return -(int)hipGetLastError();
        }
        for (int l = pl.cr_nlev - 1; l >= 0; l--) {
            const int e0 = eptr[l], ne = eptr[l + 1] - e0;
            KT_B(d);
            k_cr32_back<<<ne, 256, 0, d->stream>>>(c->cr_elim + 3 * e0, n32, TB, d->ld,
                                                   c->linv, c->crL, c->ywork, d->da);
            KT_E(d, KT_CR_BACK);
        }
        return -(int)hipGetLastError();
    }
    if (pl.cr_nlev > 0) {   // (status cleared by k_assemble_tiles)
        // one workgroup per CU (LDS): fan a level out over 5 (factor) / 4
        // (update) workgroups per tile while that still fits in one wave of
        // workgroups -- the levels are latency bound, the chip mostly idle
        const int ncu = d->ncu;
        for (int l = 0; l < pl.cr_nlev; l++) {
            const int e0 = eptr[l], ne = eptr[l + 1] - e0;
            const int k0 = kptr[l], nk = kptr[l + 1] - k0;
            const int fs = 5 * ne <= ncu, us = 4 * nk <= ncu;
            KT_B(d);
            k_cr_factor<<<fs ? 5 * ne : ne, 256, smem3, d->stream>>>(
                c->S, d->lds, c->cr_elim + 3 * e0, nt, c->linv, c->crL, d->rhs, c->ywork,
                d->scal + 4, fs);
            KT_E(d, KT_CR_FACTOR);
            if (nk > 0) {
                KT_B(d);
                k_cr_update<<<us ? 4 * nk : nk, 256, smem3, d->stream>>>(
                    c->S, d->lds, c->cr_keep + 4 * k0, nt, c->crL, d->rhs, c->ywork, us);
                KT_E(d, KT_CR_UPDATE);
            }
        }
        for (int l = pl.cr_nlev - 1; l >= 0; l--) {
            const int e0 = eptr[l], ne = eptr[l + 1] - e0;
            KT_B(d);
            k_cr_back<<<ne, 256, 0, d->stream>>>(c->cr_elim + 3 * e0, nt, c->linv, c->crL,
                                                 c->ywork, d->da);
            KT_E(d, KT_CR_BACK);
        }
        return -(int)hipGetLastError();
    }
    // the envelope factor's in-launch hand-off (not in a re-solve)
    unsigned *kflag = nospin ? nullptr : c->kflag;
    if (kflag && ++c->fac_epoch == 0) c->fac_epoch = 1;
    if (pl.nd_np > 0) {   // nested dissection: the arcs side by side, then the separator
        const int np = pl.nd_np, s0 = pl.nd_a0[np];
        const long long L = pl.slds;
        TRY_RC(ba_ensure_dyn_lds((const void *)k_factor_multi, smem3));
        int nsteps = 0;
        for (int t = 0; t < np; t++) nsteps = std::max(nsteps, pl.nd_a0[t + 1] - pl.nd_a0[t]);
        bool run = env_run_on(d, kflag, nsteps);
        if (run) {
            env_runs Rn{};
            Rn.np = np;
            for (int t = 0; t < np; t++) {
                Rn.k0[t] = pl.nd_a0[t];
                Rn.k1[t] = pl.nd_a0[t + 1];
            }
            if (env_runner_start(d, Rn, L, c->nd_rhs)) run = false;   // the launches alone
        }
        for (int st = 0; st < nsteps; st++) {
            nd_step P;
            chol_nd_step(pl, st, run, &P);
            const int nbk = P.b0[P.np];
            KT_B(d);
            k_factor_multi<<<nbk, 256, kflag ? sizeof(double) * 2 * NB * LP : smem3, d->stream>>>(
                c->S, L, c->pan_list, P, s0, c->linv, c->nd_rhs, c->ywork, d->scal + 4, kflag,
                c->fac_epoch, env_rm_of(d, 0));
            KT_E(d, KT_FACTOR);
        }
        if (run) VLGBA_CHECK(hipStreamWaitEvent(d->stream, d->ev_join, 0));
        if (pl.nd_nrec > 0) {
            const size_t smem2 = sizeof(double) * 2 * NB * LP;
            TRY_RC(ba_ensure_dyn_lds((const void *)k_sep_update, smem2));
            KT_B(d);
            k_sep_update<<<pl.nd_nrec, 256, smem2, d->stream>>>(
                c->S, L, c->nd_pair, c->nd_rec, c->nd_klist, c->ywork, c->nd_part);
            k_sep_reduce<<<pl.nd_npair, 256, 0, d->stream>>>(c->S, L, c->nd_pair, c->nd_pptr,
                                                             c->nd_part, c->nd_rhs);
            KT_E(d, KT_SYRK);
        }
        TRY_RC(envelope_columns(d, s0, nt, L, c->nd_rhs, kflag));
        TRY_RC(envelope_backward(d, L, c->nd_x, nospin));
        k_nd_scatter<<<(int)((d->lds + 255) / 256), 256, 0, d->stream>>>(c->nd_prow, c->nd_x,
                                                                         d->da, d->lds);
        return -(int)hipGetLastError();
    }
    TRY_RC(envelope_columns(d, 0, nt, d->lds, d->rhs, kflag));
    TRY_RC(envelope_backward(d, d->lds, d->da, nospin));
    return -(int)hipGetLastError();
}
