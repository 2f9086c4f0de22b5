/*
 * ba_small_solve.h -- the NA x NA solve of the one-camera pass (k_resect_pass,
 * lane 0), host and device: da = pinv(S) e_ of bundle_euclid.m:193 for S = U*
 * (fix_structure zeroes V, W, eB, so V*^-1 = pinv(0) = 0, Y = 0 and e_ = eA:
 * :140-193).  Include from C++ or HIP.
 */
#ifndef BA_SMALL_SOLVE_H
#define BA_SMALL_SOLVE_H

#include "vlg_math.h"

/* inlined into the pass: lane 0 runs it on the kernel's LDS arrays */
#define SMALL_SOLVE_HD VLG_HD __attribute__((always_inline))

/* S (NA x NA column major, the lower triangle is read) and rhs, both changed in
 * place by the pinv rule for exactly-zero rows (App. A Q2 / Q8: unit diagonal,
 * zero rhs); then the sequential Cholesky of the lower triangle with its two
 * substitutions (the parity-mode solve's loops), or, on a pivot that is not
 * positive, cyclic Jacobi on the symmetrised S with MATLAB's tolerance
 * NA * eps(max |eigenvalue|).  Returns 1 when da came from that fallback. */
template <int NA>
SMALL_SOLVE_HD int small_solve(double *S, double *rhs, double *da)
{
    for (int j = 0; j < NA; j++)
        if (S[j + NA * j] == 0.0) {
            S[j + NA * j] = 1.0;
            rhs[j] = 0.0;
        }
    double L[NA * NA];
    for (int q = 0; q < NA * NA; q++) L[q] = S[q];
    bool ok = true;
    for (int j = 0; j < NA && ok; j++) {
        double s = L[j + NA * j];
        for (int k = 0; k < j; k++) s = s - L[j + NA * k] * L[j + NA * k];
        if (!(s > 0.0)) {
            ok = false;
            break;
        }
        const double p = sqrt(s);
        L[j + NA * j] = p;
        for (int i = j + 1; i < NA; i++) {
            double t = L[i + NA * j];
            for (int k = 0; k < j; k++) t = t - L[i + NA * k] * L[j + NA * k];
            L[i + NA * j] = t / p;
        }
    }
    if (ok) {
        double x[NA];
        for (int i = 0; i < NA; i++) {
            double t = rhs[i];
            for (int k = 0; k < i; k++) t = t - L[i + NA * k] * x[k];
            x[i] = t / L[i + NA * i];
        }
        for (int i = NA - 1; i >= 0; i--) {
            double t = x[i];
            for (int k = i + 1; k < NA; k++) t = t - L[k + NA * i] * x[k];
            x[i] = t / L[i + NA * i];
        }
        for (int i = 0; i < NA; i++) da[i] = x[i];
        return 0;
    }
    /* da = pinv(S) e_ (bundle_euclid.m:193) */
    double A[NA][NA], Q[NA][NA];
    for (int p = 0; p < NA; p++)
        for (int q = 0; q < NA; q++) {
            const double sp = p >= q ? S[p + NA * q] : S[q + NA * p];
            A[p][q] = sp;
            Q[p][q] = p == q ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0;
        for (int p = 0; p < NA; p++)
            for (int q = p + 1; q < NA; q++) off += A[p][q] * A[p][q];
        if (off == 0.0) break;
        for (int p = 0; p < NA - 1; p++)
            for (int q = p + 1; q < NA; q++) {
                if (A[p][q] == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < NA; k++) {
                    const double u = A[k][p], v = A[k][q];
                    A[k][p] = c * u - sn * v;
                    A[k][q] = sn * u + c * v;
                }
                for (int k = 0; k < NA; k++) {
                    const double u = A[p][k], v = A[q][k];
                    A[p][k] = c * u - sn * v;
                    A[q][k] = sn * u + c * v;
                }
                for (int k = 0; k < NA; k++) {
                    const double u = Q[k][p], v = Q[k][q];
                    Q[k][p] = c * u - sn * v;
                    Q[k][q] = sn * u + c * v;
                }
            }
    }
    double emax = 0.0;
    for (int k = 0; k < NA; k++) emax = fmax(emax, fabs(A[k][k]));
    int e;
    (void)frexp(emax, &e);
    const double tol = emax > 0.0 ? NA * ldexp(1.0, e - 53) : 0.0;
    double x[NA] = {};
    for (int k = 0; k < NA; k++) {
        if (!(fabs(A[k][k]) > tol)) continue;
        double w = 0.0;
        for (int i = 0; i < NA; i++) w += Q[i][k] * rhs[i];
        w /= A[k][k];
        for (int i = 0; i < NA; i++) x[i] += Q[i][k] * w;
    }
    for (int i = 0; i < NA; i++) da[i] = x[i];
    return 1;
}

/* the pass's call: S = U with the diagonal times 1 + lambda, rhs = eA from the
 * kept state st = U | eA (bundle_euclid.m:162-173), then small_solve */
template <int NA>
SMALL_SOLVE_HD int small_solve_damped(const double *st, double lambda, double *S, double *rhs,
                                      double *da)
{
    for (int c = 0; c < NA; c++)
        for (int r = 0; r < NA; r++) {
            const double u = st[r + NA * c];
            S[r + NA * c] = (r == c) ? (1 + lambda) * u : u;
        }
    for (int r = 0; r < NA; r++) rhs[r] = st[NA * NA + r];
    return small_solve<NA>(S, rhs, da);
}

#endif /* BA_SMALL_SOLVE_H */
