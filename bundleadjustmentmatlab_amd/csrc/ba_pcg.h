// ba_pcg.h -- the state of the block-Jacobi PCG reduced solve (internal to
// libvlgba.so; dense_solve = 5).  One ba_pcg per such context, owned by
// ba_pcg_setup / ba_pcg_free through ba_dev::pcg; such a context has no ba_chol
// (ba_dev::chol is null: no dense S, no plan of the direct solves).
#pragma once
#include <hip/hip_runtime.h>

// camera rows per 256-thread workgroup of every PCG kernel (one wave each);
// the dot products' partial sums are per workgroup
#define BA_PCG_ROWS 4
// iterations enqueued before the host reads the done word: the first batch,
// doubled per batch up to the cap
#define BA_PCG_BATCH0 8
#define BA_PCG_BATCH_MAX 64

// the scalars of the recurrences, on the device for the whole solve
struct ba_pcg_state {
    double rz0;       // r' M^-1 r at da = 0
    double rz[2];     // ... entering iteration k, at [k & 1]
    double relres;    // sqrt(rz_k / rz_0) after the last iteration run
    int done[2];      // iteration k returns at once when done[k & 1]
    int iters;        // iterations run
    int conv;         // relres <= tol
    int fail;         // this iteration's p'Sp was not positive (k_pcg_update)
    int pad[3];       // (64 bytes)
};

struct ba_pcg {
    // settings and the last solve's statistics (host; vlgba_set_pcg, vlgba_get_pcg_stats)
    double tol;
    int max_iter;
    int iters, conv;
    double relres;
    long long total;
    // block CSR over both triangles (pcg_plan, ba_chol_plan.h); ent / nbr hold
    // 2 nb entries' room (nnz <= 2 nb)
    int nnz, nwg;               // entries; workgroups = ceil(m / BA_PCG_ROWS)
    int *rowptr, *ent, *nbr, *dblk;
    // work vectors r | z | p | q, [ld] each (the iterate is ba_dev::da)
    double *vec;
    double *minv;               // [m][na * na] M_j^-1, column major, symmetric
    unsigned char *fixed;       // [ld] the exactly-zero rows (da = 0 there)
    double *part;               // [2][nwg] partial sums: p'q | r'z per workgroup
    ba_pcg_state *st;
    long long bytes;            // of the above (vlgba_plan_info [32])
};
