/*
 * ba_triang_math.h -- the per-point arithmetic of ba_triang.hip (linear
 * triangulation and the one-point LM pass with the motion fixed), host and
 * device: the kernels are thin loops around these, and tests/native/
 * block_host.cpp runs the same code on the CPU.  Include from C++ or HIP.
 *
 * Camera records (k_tri_cameras writes them once per call):
 *   TRI_CAM doubles per camera:  P (12, 3 x 4 column major:
 *   calibration_matrix(K) [R(w) T]) | K4 (4) | R(w) (9) | T (3)
 * Radial lenses (vlgba_triangulate_ex, vlgba_intersect_ex): the record is the
 * pinhole one with K4 = (f, f, cx, cy); k1, k2 travel in a side array kd (2 per
 * camera), so the pinhole record and its arithmetic stay what they were.
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
VLG_HD int tri_solve(const double G[10], long long nv, const int *cam, const double *rec,
                     double X[4]);

VLG_HD int tri_undistort(double f, const double c[2], double k1, double k2, const double x[2],
                         double n[2]);

/* RADIAL = false: kd is not read.  RADIAL = true, radial lenses (kd: k1, k2 per
 * camera; f = K4[0], the principal point K4[2], K4[3] of the record, whose P
 * was formed with K = (f, f, cx, cy)): every measurement is undistorted to the
 * pinhole pixel f n + c first, then the rows are the same.  A view that
 * tri_undistort fails gives the point status 2 and zeros. */
template <bool RADIAL>
VLG_HD int tri_point(long long nv, const int *cam, const double *x, const double *rec,
                     const double *kd, double X[4])
{
    double G[10];
    long long o;
    int c;
    X[0] = X[1] = X[2] = X[3] = 0.0;
    if (nv < 2) return 2;
    for (c = 0; c < 10; c++) G[c] = 0.0;
    for (o = 0; o < nv; o++) {
        const double *rc = rec + (size_t)TRI_CAM * cam[o];
        if (RADIAL) {
            const double *k4 = rc + TRI_CAM_K4;
            double n[2];
            if (!tri_undistort(k4[0], k4 + 2, kd[2 * (size_t)cam[o]], kd[2 * (size_t)cam[o] + 1],
                               x + 2 * o, n))
                return 2;
            tri_add_view(G, rc, k4[0] * n[0] + k4[2], k4[0] * n[1] + k4[3]);
        } else {
            tri_add_view(G, rc, x[2 * o], x[2 * o + 1]);
        }
    }
    return tri_solve(G, nv, cam, rec, X);
}

/* Undistortion of one measurement x under the radial lens (f, k1, k2,
 * principal point c): nd = (x - c) / f, rd = |nd|; solve r (1 + k1 r^2 +
 * k2 r^4) = rd by Newton from r = rd, then n = nd (r / rd), n = 0 at rd = 0.
 * At most TRI_UNDIST_ITERS updates; settled when an update changes r by no
 * more than TRI_UNDIST_TOL |r| (8 ulps: the residual r g(r) - rd is itself
 * only good to a few ulps of rd, so a smaller update is rounding).  Returns 0
 * (the view fails) when the derivative 1 + 3 k1 r^2 + 5 k2 r^4 is <= 0 at any
 * iterate or at the settled r (at or past the fold of the lens, where the
 * distortion stops being invertible), when the iteration does not settle, and
 * for a non-finite result; 1 otherwise. */
#define TRI_UNDIST_ITERS 20
#define TRI_UNDIST_TOL 0x1p-49
VLG_HD int tri_undistort(double f, const double c[2], double k1, double k2, const double x[2],
                         double n[2])
{
    const double nd0 = (x[0] - c[0]) / f, nd1 = (x[1] - c[1]) / f;
    const double rd = sqrt(nd0 * nd0 + nd1 * nd1);
    double r = rd, r2, dg;
    int it, ok = 0;
    n[0] = n[1] = 0.0;
    if (rd == 0.0) return 1;
    for (it = 0; it < TRI_UNDIST_ITERS && !ok; it++) {
        double g, dr;
        r2 = r * r;
        g = (1.0 + k1 * r2) + (k2 * r2) * r2;
        dg = (1.0 + 3.0 * (k1 * r2)) + 5.0 * ((k2 * r2) * r2);
        if (!(dg > 0.0)) return 0;
        dr = (r * g - rd) / dg;
        r = r - dr;
        ok = fabs(dr) <= TRI_UNDIST_TOL * fabs(r);
    }
    r2 = r * r;
    dg = (1.0 + 3.0 * (k1 * r2)) + 5.0 * ((k2 * r2) * r2);
    if (!ok || !(dg > 0.0) || !(r > 0.0) || !(r <= 1.79769313486231570e308)) return 0;
    n[0] = nd0 * (r / rd);
    n[1] = nd1 * (r / rd);
    return 1;
}

/* the point from the Gram matrix of its rows: X (zeros unless status 1) */
VLG_HD int tri_solve(const double G[10], long long nv, const int *cam, const double *rec,
                     double X[4])
{
    double v[4];
    long long o;
    int st = 1;
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

/* The mode of vlgba_intersect_ex.  kd: NULL pinhole, else k1, k2 per camera
 * (radial lens, f = K4[0], principal point K4[2], K4[3]: vlg_project_radial);
 * jac: 0 forward differences, 1 the closed-form B; loss / c: vlg_loss.  The
 * pass is a template over M: M = false is vlgba_intersect's (the mode is not
 * read, every branch on it folds away); M = true with kd NULL, jac 0, loss 0
 * performs the same operations in the same order. */
typedef struct {
    const double *kd;
    int jac, loss;
    double c;
} isect_mode;

VLG_HD void isect_project_m(const double *rc, const double *k12, const double b[3], double x[2])
{
    if (k12) {
        const double k[3] = {rc[TRI_CAM_K4], k12[0], k12[1]};
        vlg_project_radial(k, rc + TRI_CAM_K4 + 2, rc + TRI_CAM_R, rc + TRI_CAM_T, b, x);
    } else {
        isect_project(rc, b, x);
    }
}

/* B = dx/db in closed form (column k at B[2k], B[2k+1]): the B columns of
 * cam_view<6>::jac_columns and cam_view<BA_RAD_NA>::jac_columns (ba_camera.h)
 * restated for host and device, operation for operation */
VLG_HD void isect_jac_B(const double *rc, const double *k12, const double b[3], double B[6])
{
    const double *R = rc + TRI_CAM_R, *T = rc + TRI_CAM_T;
    int k;
    if (k12) {
        const double kk[3] = {rc[TRI_CAM_K4], k12[0], k12[1]};
        double n[2], iz, r2, d;
        vlg_radial_n(kk, R, T, b, n, &iz, &r2, &d);
        {
            const double f = kk[0], u = n[0], v = n[1];
            const double g = 2.0 * kk[1] + 4.0 * (kk[2] * r2);
            const double fd = f * d, fgu = (f * g) * u, fgv = (f * g) * v;
            for (k = 0; k < 3; k++) {
                const double p0 = iz * (R[3 * k] - u * R[3 * k + 2]);
                const double p1 = iz * (R[3 * k + 1] - v * R[3 * k + 2]);
                const double s = u * p0 + v * p1;
                B[2 * k] = fd * p0 + fgu * s;
                B[2 * k + 1] = fd * p1 + fgv * s;
            }
        }
    } else {
        double S[3];
        vlg_rot_b(R, b, S);
        {
            const double X0 = S[0] + T[0], X1 = S[1] + T[1], z = S[2] + T[2];
            const double iz = 1.0 / z;
            const double u = X0 * iz, v = X1 * iz;
            const double fxz = rc[TRI_CAM_K4] * iz, fyz = rc[TRI_CAM_K4 + 1] * iz;
            for (k = 0; k < 3; k++) {
                B[2 * k] = fxz * (R[3 * k] - u * R[3 * k + 2]);
                B[2 * k + 1] = fyz * (R[3 * k + 1] - v * R[3 * k + 2]);
            }
        }
    }
}

/* one residual's term of the (robust) cost, added as the plain pass adds it
 * when it is the plain term (vlg_loss_plain) */
template <bool M>
VLG_HD double isect_cost_add(double acc, const isect_mode *md, double e0, double e1)
{
    const double s = e0 * e0 + e1 * e1;
    if (!M || vlg_loss_plain(md->loss, md->c, s)) {
        acc = acc + e0 * e0;
        acc = acc + e1 * e1;
    } else {
        double rho, sw;
        vlg_loss(md->loss, md->c, s, &rho, &sw);
        acc = acc + rho;
    }
    return acc;
}

/* linearise at b (mex_bundle_1_XABeUVWeAeB.c:43-70, 196-225, 280-332 for this
 * point's columns): V = sum B'B, eB = sum B'e and e(:)'e(:) in view order */
template <bool M>
VLG_HD void isect_linearize(long long nv, const int *cam, const double *x, const double *rec,
                            const isect_mode *md, const double b[3], double st[TRI_NST])
{
    long long o;
    int r, c, k;
    for (k = 0; k < TRI_NST; k++) st[k] = 0.0;
    for (o = 0; o < nv; o++) {
        const double *rc = rec + (size_t)TRI_CAM * cam[o];
        const double *k12 = M && md->kd ? md->kd + 2 * (size_t)cam[o] : 0;
        double xh[2], B[6], e[2], u[2];
        isect_project_m(rc, k12, b, xh);
        if (M && md->jac) {
            isect_jac_B(rc, k12, b, B);
        } else {
            for (k = 0; k < 3; k++) {
                double b1[3], x1[2];
                for (c = 0; c < 3; c++) b1[c] = b[c] + VLG_FD_H * ((c == k) ? 1.0 : 0.0);
                isect_project_m(rc, k12, b1, x1);
                B[2 * k] = vlg_fd_quot(x1[0] - xh[0]);
                B[2 * k + 1] = vlg_fd_quot(x1[1] - xh[1]);
            }
        }
        u[0] = e[0] = x[2 * o] - xh[0];
        u[1] = e[1] = x[2 * o + 1] - xh[1];
        if (M && md->loss) {   /* the rows [B | e] times sqrt(w), where they are formed */
            double rho, sw;
            vlg_loss(md->loss, md->c, e[0] * e[0] + e[1] * e[1], &rho, &sw);
            for (k = 0; k < 6; k++) B[k] *= sw;
            e[0] *= sw;
            e[1] *= sw;
        }
        for (c = 0; c < 3; c++)
            for (r = 0; r < 3; r++)
                st[r + 3 * c] += B[2 * r] * B[2 * c] + B[2 * r + 1] * B[2 * c + 1];
        for (r = 0; r < 3; r++) st[9 + r] += B[2 * r] * e[0] + B[2 * r + 1] * e[1];
        st[12] = isect_cost_add<M>(st[12], md, u[0], u[1]);
    }
}

/* the step from the kept linearisation: V* (bundle_euclid.m:162-173), db =
 * V*^-1 eB (fix_motion: da = 0, so mex_bundle_3_db_new.c:99-134 subtracts exact
 * zeros), b_new = b + db, the new projections' cost and dp'(lambda dp + g) */
template <bool M>
VLG_HD void isect_step(long long nv, const int *cam, const double *x, const double *rec,
                       const isect_mode *md, const double b[3], const double st[TRI_NST],
                       double lambda, double bn[3], double *new_cost, double *dpg)
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
        double xh[2];
        isect_project_m(rec + (size_t)TRI_CAM * cam[o],
                        M && md->kd ? md->kd + 2 * (size_t)cam[o] : 0, bn, xh);
        ns = isect_cost_add<M>(ns, md, x[2 * o] - xh[0], x[2 * o + 1] - xh[1]);
    }
    for (r = 0; r < 3; r++) g = g + db[r] * (lambda * db[r] + st[9 + r]);
    *new_cost = ns;
    *dpg = g;
}

/* One LM pass of point i of n (the protocol of ba_batch_lm.h; k_intersect_pass's
 * lane and the host loop of tests/native/block_host.cpp): fl and lambda are the
 * point's flags word and lambda of this pass, b / b_new its two parameter sets
 * (3 n each), state (SoA, entry k of point i at state[k * n + i]) V | eB | old
 * cost, kept across rejected passes (bundle_euclid.m:139 recomputes an
 * identical linearisation, Q12), out the four scalars per point. */
template <bool M>
VLG_HD void isect_pass_point(long long i, long long n, const long long *obs_ptr,
                             const int *obs_cam, const double *obs_x, const double *rec,
                             const isect_mode *md, double *b, double *b_new, double *state,
                             int fl, double lambda, double *out)
{
    if (!(fl & 1)) return;   /* point finished (or without views) */
    const long long o0 = obs_ptr[i], nv = obs_ptr[i + 1] - o0;
    const int *cam = obs_cam + o0;
    const double *x = obs_x + 2 * o0;
    double bv[3], st[TRI_NST], bn[3], nsum, g;
    int c, k;
    if (fl & 4)              /* the previous pass was accepted */
        for (c = 0; c < 3; c++) b[3 * i + c] = b_new[3 * i + c];
    for (c = 0; c < 3; c++) bv[c] = b[3 * i + c];
    if (fl & 2) {
        isect_linearize<M>(nv, cam, x, rec, md, bv, st);
        for (k = 0; k < TRI_NST; k++) state[(size_t)k * n + i] = st[k];
    } else {
        for (k = 0; k < TRI_NST; k++) st[k] = state[(size_t)k * n + i];
    }
    isect_step<M>(nv, cam, x, rec, md, bv, st, lambda, bn, &nsum, &g);
    for (c = 0; c < 3; c++) b_new[3 * i + c] = bn[c];
    out[4 * i + 0] = st[12];
    out[4 * i + 1] = nsum;
    out[4 * i + 2] = g;
    out[4 * i + 3] = 0.0;   /* no pinv fallback: vlg_pinv3 is the solve */
}

/* the unweighted residuals x - x_hat (2 per view) and the loss's weights (1 per
 * view; sqrt(w) squared, 1 without a loss) of one point at b; either may be 0 */
VLG_HD void isect_residuals_m(long long nv, const int *cam, const double *x, const double *rec,
                              const isect_mode *md, const double b[3], double *res, double *w)
{
    long long o;
    for (o = 0; o < nv; o++) {
        double xh[2], e0, e1, rho, sw;
        isect_project_m(rec + (size_t)TRI_CAM * cam[o],
                        md->kd ? md->kd + 2 * (size_t)cam[o] : 0, b, xh);
        e0 = x[2 * o] - xh[0];
        e1 = x[2 * o + 1] - xh[1];
        vlg_loss(md->loss, md->c, e0 * e0 + e1 * e1, &rho, &sw);
        if (res) {
            res[2 * o] = e0;
            res[2 * o + 1] = e1;
        }
        if (w) w[o] = sw * sw;
    }
}

#endif /* BA_TRIANG_MATH_H */
