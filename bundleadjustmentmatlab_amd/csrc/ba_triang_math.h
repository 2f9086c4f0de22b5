/*
 * ba_triang_math.h -- the per-point arithmetic of ba_triang.hip (linear
 * triangulation and the one-point LM pass with the motion fixed), host and
 * device: the kernels are thin loops around these, and a CPU build can run the
 * same code.  Include from C++ or HIP.
 *
 * Camera records (k_tri_cameras writes them once per call):
 *   TRI_CAM doubles per camera:  P (12, 3 x 4 column major:
 *   calibration_matrix(K) [R(w) T]) | K4 (4) | R(w) (9) | T (3)
 */
#ifndef BA_TRIANG_MATH_H
#define BA_TRIANG_MATH_H

#include "vlg_math.h"

#define TRI_CAM 28
#define TRI_CAM_K4 12
#define TRI_CAM_R 16
#define TRI_CAM_T 25
/* state of a point across rejected passes: V (9) | eB (3) | old SSE */
#define TRI_NST 13

/* one camera's record: R = vl_rodrigues(w) (the rotation table's slot 0, bit
 * for bit), P = calibration_matrix(K) [R T] (triangulation.m:24-27) */
VLG_HD void tri_camera(const double K4[4], const double T[3], const double w[3], double *rec)
{
    double R[9];
    int c;
    vlg_rodrigues(R, w);
    for (c = 0; c < 4; c++) {
        const double r0 = c < 3 ? R[3 * c] : T[0];
        const double r1 = c < 3 ? R[3 * c + 1] : T[1];
        const double r2 = c < 3 ? R[3 * c + 2] : T[2];
        rec[3 * c] = K4[0] * r0 + K4[2] * r2;
        rec[3 * c + 1] = K4[1] * r1 + K4[3] * r2;
        rec[3 * c + 2] = r2;
    }
    for (c = 0; c < 4; c++) rec[TRI_CAM_K4 + c] = K4[c];
    for (c = 0; c < 9; c++) rec[TRI_CAM_R + c] = R[c];
    for (c = 0; c < 3; c++) rec[TRI_CAM_T + c] = T[c];
}

/* G += r r' for one row r of A (the upper triangle, 10 entries:
 * 00 01 02 03 11 12 13 22 23 33) */
VLG_HD void tri_gram_row(double G[10], const double r[4])
{
    G[0] += r[0] * r[0]; G[1] += r[0] * r[1]; G[2] += r[0] * r[2]; G[3] += r[0] * r[3];
    G[4] += r[1] * r[1]; G[5] += r[1] * r[2]; G[6] += r[1] * r[3];
    G[7] += r[2] * r[2]; G[8] += r[2] * r[3];
    G[9] += r[3] * r[3];
}

/* the two rows u P3 - P1, v P3 - P2 of one view (triangulation.m:36-37) */
VLG_HD void tri_add_view(double G[10], const double *P, double u, double v)
{
    double r0[4], r1[4];
    int c;
    for (c = 0; c < 4; c++) {
        r0[c] = u * P[3 * c + 2] - P[3 * c];
        r1[c] = v * P[3 * c + 2] - P[3 * c + 1];
    }
    tri_gram_row(G, r0);
    tri_gram_row(G, r1);
}

/* one Jacobi rotation of the symmetric 4 x 4 a (full storage) in the (p, q)
 * plane, accumulated into the eigenvector matrix z (columns); p < q constants
 * after unrolling, so a and z stay in registers */
#define TRI_ROT(p, q)                                                              \
    do {                                                                           \
        const double apq = a[p][q];                                                \
        if (apq != 0.0) {                                                          \
            const double th = (a[q][q] - a[p][p]) / (2.0 * apq);                   \
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0)); \
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                   \
            int k_;                                                                \
            for (k_ = 0; k_ < 4; k_++) {                                           \
                const double x_ = a[k_][p], y_ = a[k_][q];                         \
                a[k_][p] = c * x_ - s * y_;                                        \
                a[k_][q] = s * x_ + c * y_;                                        \
            }                                                                      \
            for (k_ = 0; k_ < 4; k_++) {                                           \
                const double x_ = a[p][k_], y_ = a[q][k_];                         \
                a[p][k_] = c * x_ - s * y_;                                        \
                a[q][k_] = s * x_ + c * y_;                                        \
            }                                                                      \
            a[p][q] = 0.0;                                                         \
            a[q][p] = 0.0;                                                         \
            for (k_ = 0; k_ < 4; k_++) {                                           \
                const double x_ = z[k_][p], y_ = z[k_][q];                         \
                z[k_][p] = c * x_ - s * y_;                                        \
                z[k_][q] = s * x_ + c * y_;                                        \
            }                                                                      \
        }                                                                          \
    } while (0)

/* eigenvector of the smallest eigenvalue of the Gram matrix G = A'A (cyclic
 * Jacobi: the right singular vector of A's smallest singular value,
 * triangulation.m:41-42).  Sweeps end when the off-diagonal mass is below
 * 1e-40 of the diagonal's (1e-20 in norm: far under the rounding of G itself;
 * Jacobi converges quadratically, so that is one sweep past 1e-10). */
VLG_HD void tri_smallest_vec(const double G[10], double v[4])
{
    double a[4][4], z[4][4];
    int i, j, sweep;
    a[0][0] = G[0]; a[0][1] = G[1]; a[0][2] = G[2]; a[0][3] = G[3];
    a[1][1] = G[4]; a[1][2] = G[5]; a[1][3] = G[6];
    a[2][2] = G[7]; a[2][3] = G[8];
    a[3][3] = G[9];
    for (i = 0; i < 4; i++)
        for (j = 0; j < 4; j++) {
            if (j < i) a[i][j] = a[j][i];
            z[i][j] = i == j ? 1.0 : 0.0;
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (sweep = 0; sweep < 24; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] +
                           a[1][2] * a[1][2] + a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dg = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] +
                          a[3][3] * a[3][3];
        if (!(off > 1e-40 * dg)) break;
        TRI_ROT(0, 1);
        TRI_ROT(0, 2);
        TRI_ROT(0, 3);
        TRI_ROT(1, 2);
        TRI_ROT(1, 3);
        TRI_ROT(2, 3);
    }
    {
        /* column of the smallest diagonal entry, by selects (no indexed access) */
        double d = a[0][0];
        for (i = 0; i < 4; i++) v[i] = z[i][0];
        if (a[1][1] < d) {
            d = a[1][1];
            for (i = 0; i < 4; i++) v[i] = z[i][1];
        }
        if (a[2][2] < d) {
            d = a[2][2];
            for (i = 0; i < 4; i++) v[i] = z[i][2];
        }
        if (a[3][3] < d) {
            d = a[3][3];
            for (i = 0; i < 4; i++) v[i] = z[i][3];
        }
    }
}

/* point of nv views (camera ids cam[], measurements x[2 * .]) from the camera
 * records: X (4) and the status 1 triangulated / 0 behind a camera / 2 fewer
 * than two views or a non-finite result (X zeros unless 1) */
VLG_HD int tri_point(long long nv, const int *cam, const double *x, const double *rec, double X[4])
{
    double G[10], v[4];
    long long o;
    int c, st = 1;
    X[0] = X[1] = X[2] = X[3] = 0.0;
    if (nv < 2) return 2;
    for (c = 0; c < 10; c++) G[c] = 0.0;
    for (o = 0; o < nv; o++)
        tri_add_view(G, rec + (size_t)TRI_CAM * cam[o], x[2 * o], x[2 * o + 1]);
    tri_smallest_vec(G, v);
    {
        const double x0 = v[0] / v[3], x1 = v[1] / v[3], x2 = v[2] / v[3];
        /* v(4) == 0 (a point at infinity) gives inf / nan here: status 2 */
        if (!(fabs(x0) <= 1.79769313486231570e308 && fabs(x1) <= 1.79769313486231570e308 &&
              fabs(x2) <= 1.79769313486231570e308))
            return 2;
        /* depth test (triangulation.m:46-52): P_j(3,:) X < 0 in any view */
        for (o = 0; o < nv; o++) {
            const double *P = rec + (size_t)TRI_CAM * cam[o];
            const double d = P[2] * x0 + P[5] * x1 + P[8] * x2 + P[11];
            if (d < 0.0) st = 0;
        }
        if (st == 1) {
            X[0] = x0; X[1] = x1; X[2] = x2; X[3] = 1.0;
        }
    }
    return st;
}

/* ---- one LM pass of one point, the cameras fixed ---------------------------
 * projection of b in the camera of record rc (reproject_point.h:16-57, K not
 * variable, R(w) from the record) */
VLG_HD void isect_project(const double *rc, const double b[3], double x[2])
{
    double Kc[9];
    vlg_calib(Kc, rc + TRI_CAM_K4, rc, 0);
    vlg_project(Kc, rc + TRI_CAM_R, rc + TRI_CAM_T, b, x);
}

/* linearise at b (mex_bundle_1_XABeUVWeAeB.c:43-70, 196-225, 280-332 for this
 * point's columns): V = sum B'B, eB = sum B'e and e(:)'e(:) in view order */
VLG_HD void isect_linearize(long long nv, const int *cam, const double *x, const double *rec,
                            const double b[3], double st[TRI_NST])
{
    long long o;
    int r, c, k;
    for (k = 0; k < TRI_NST; k++) st[k] = 0.0;
    for (o = 0; o < nv; o++) {
        const double *rc = rec + (size_t)TRI_CAM * cam[o];
        double xh[2], B[6], e[2];
        isect_project(rc, b, xh);
        for (k = 0; k < 3; k++) {
            double b1[3], x1[2];
            for (c = 0; c < 3; c++) b1[c] = b[c] + VLG_FD_H * ((c == k) ? 1.0 : 0.0);
            isect_project(rc, b1, x1);
            B[2 * k] = vlg_fd_quot(x1[0] - xh[0]);
            B[2 * k + 1] = vlg_fd_quot(x1[1] - xh[1]);
        }
        e[0] = x[2 * o] - xh[0];
        e[1] = x[2 * o + 1] - xh[1];
        for (c = 0; c < 3; c++)
            for (r = 0; r < 3; r++)
                st[r + 3 * c] += B[2 * r] * B[2 * c] + B[2 * r + 1] * B[2 * c + 1];
        for (r = 0; r < 3; r++) st[9 + r] += B[2 * r] * e[0] + B[2 * r + 1] * e[1];
        st[12] = st[12] + e[0] * e[0];
        st[12] = st[12] + e[1] * e[1];
    }
}

/* the step from the kept linearisation: V* (bundle_euclid.m:162-173), db =
 * V*^-1 eB (fix_motion: da = 0, so mex_bundle_3_db_new.c:99-134 subtracts exact
 * zeros), b_new = b + db, the new projections' e'e and dp'(lambda dp + g) */
VLG_HD void isect_step(long long nv, const int *cam, const double *x, const double *rec,
                       const double b[3], const double st[TRI_NST], double lambda,
                       double bn[3], double *new_sse, double *dpg)
{
    double Vs[9], Vi[9], db[3], ns = 0.0, g = 0.0;
    long long o;
    int r, k;
    for (k = 0; k < 9; k++) Vs[k] = st[k];
    for (k = 0; k < 3; k++) Vs[4 * k] = (1 + lambda) * st[4 * k];
    vlg_pinv3(Vs, Vi);
    for (r = 0; r < 3; r++)
        db[r] = Vi[r] * st[9] + Vi[r + 3] * st[10] + Vi[r + 6] * st[11];
    for (r = 0; r < 3; r++) bn[r] = b[r] + db[r];
    for (o = 0; o < nv; o++) {
        double xh[2], d0, d1;
        isect_project(rec + (size_t)TRI_CAM * cam[o], bn, xh);
        d0 = x[2 * o] - xh[0];
        d1 = x[2 * o + 1] - xh[1];
        ns = ns + d0 * d0;
        ns = ns + d1 * d1;
    }
    for (r = 0; r < 3; r++) g = g + db[r] * (lambda * db[r] + st[9 + r]);
    *new_sse = ns;
    *dpg = g;
}

#endif /* BA_TRIANG_MATH_H */
