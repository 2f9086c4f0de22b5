// ba_camera.h -- device view of one camera for the projections of the
// linearisation kernels (ba_kernels.hip) and the batched resection
// (ba_resect.hip): the reference's reproject_point.h:16-57 with the per-camera
// rotations hoisted into a table (vl_rodrigues).
#pragma once
#include "ba_internal.h"
#include "vlg_math.h"

#define H_FD VLG_FD_H

// -------------------------------------------------------------------------
// camera j as the projections see it.  Euclidean (NA = 6 / 7 / 10): a0, the
// calibration of reproject_point.h:26-41 and the hoisted rotations
// R(w), R(w + h e_k), R(w + 0) (k_rotations); projective (NA = BA_PROJ_NA):
// P = a0 (mex_bundle_proj_1_XABeUVWeAeB.c:21-22), K4 / rot unused; radial
// distortion (NA = BA_RAD_NA): a0, the principal point and R(w), dR/dw_k.
//   project(b, x)         x = proj(a0, b)
//   project_dcam(k, b, x) x = proj(a0 + h e_k, b), a1 formed component-wise
//                         as a0 + h * da (mex_bundle_1 :30-33, proj :47-51)
//   project_col(c, b, x)  column c of [A | B]: c < NA as project_dcam, else
//                         proj(a0, b + h e_{c-NA}) (mex_bundle_1 :59-66)
//   jac_columns(b, half, row)  analytic-Jacobian mode: the closed-form columns
//                         of [A | B] (rot then holds R(w), dR/dw_k, 0)
// -------------------------------------------------------------------------
template <int NA, bool PROJ = (NA == BA_PROJ_NA)>
struct cam_view;

template <int NA>
struct cam_view<NA, false> {
    double a0[NA], k4[4], Kc[9], Rl[9];
    const double *R;
    __device__ __forceinline__ cam_view(const double *__restrict__ a,
                                        const double *__restrict__ K4,
                                        const double *__restrict__ rot, int j)
        : cam_view(a, K4, rot, j, j)
    {
    }
    // jr: the camera's row of rot (a staged copy of part of the table, e.g.
    // in LDS), j: its index into a and K4
    __device__ __forceinline__ cam_view(const double *__restrict__ a,
                                        const double *__restrict__ K4,
                                        const double *__restrict__ rot, int jr, int j)
    {
#pragma unroll
        for (int c = 0; c < NA; c++) a0[c] = a[(size_t)NA * j + c];
#pragma unroll
        for (int c = 0; c < 4; c++) k4[c] = K4[4 * (size_t)j + c];
        R = rot + 45 * (size_t)jr;
#pragma unroll
        for (int q = 0; q < 9; q++) Rl[q] = R[q];
        vlg_calib(Kc, k4, a0, NA - 6);
    }
    __device__ __forceinline__ void project(const double b[3], double x[2]) const
    {
        vlg_project(Kc, Rl, a0 + 3, b, x);
    }
    __device__ __forceinline__ void project_dcam(int k, const double b[3], double x[2]) const
    {
        double a1[NA], Kc1[9], Rk[9];
#pragma unroll
        for (int c = 0; c < NA; c++) a1[c] = a0[c] + H_FD * ((c == k) ? 1.0 : 0.0);
        vlg_calib(Kc1, k4, a1, NA - 6);
        const double *Rs = R + 9 * ((k < 3) ? (1 + k) : 4);
#pragma unroll
        for (int q = 0; q < 9; q++) Rk[q] = Rs[q];
        vlg_project(Kc1, Rk, a1 + 3, b, x);
    }
    // FD column col of [A | B] without a branch: col < NA perturbs camera
    // component col (as project_dcam), col >= NA point component col - NA
    // with the unperturbed camera (mex_bundle_1 :43-70: K, R(w), T of a)
    __device__ __forceinline__ void project_col(int col, const double b[3], double x[2]) const
    {
        const bool cam = col < NA;
        double a1[NA], b1[3], Kc1[9], Rk[9];
#pragma unroll
        for (int c = 0; c < NA; c++)
            a1[c] = cam ? a0[c] + H_FD * ((c == col) ? 1.0 : 0.0) : a0[c];
#pragma unroll
        for (int c = 0; c < 3; c++)
            b1[c] = cam ? b[c] : b[c] + H_FD * ((c == col - NA) ? 1.0 : 0.0);
        vlg_calib(Kc1, k4, a1, NA - 6);
        const double *Rs = R + 9 * ((col < 3) ? (1 + col) : (cam ? 4 : 0));
#pragma unroll
        for (int q = 0; q < 9; q++) Rk[q] = Rs[q];
        vlg_project(Kc1, Rk, a1 + 3, b1, x);
    }
    // Analytic-Jacobian mode (the table's slots 1..3 hold dR/dw_k,
    // rotation_k_jac): the closed-form columns of [A | B] into row.  With
    // Xc = R b + t, z = Xc_2, u = Xc_0 / z, v = Xc_1 / z:
    //   J = dx/dXc = [fx/z 0 -fx u/z; 0 fy/z -fy v/z],  J d = (fx/z (d0 - u d2),
    //   fy/z (d1 - v d2));  A_wk = J (dR_k b), A_T = J, B = J R, and the
    //   calibration columns d x / d f = (u, v) (NA = 7), d x / d (fx fy cx cy)
    //   = (u, 0), (0, v), (1, 0), (0, 1) (NA = 10).
    // Lane 0 of the observation's pair forms the rotation columns, lane 1 the
    // rest (jac_lane1).
    __device__ __forceinline__ void jac_columns(const double b[3], int half, double *row) const
    {
        double S[3];
        vlg_rot_b(Rl, b, S);
        const double X0 = S[0] + a0[3], X1 = S[1] + a0[4], z = S[2] + a0[5];
        const double iz = 1.0 / z;
        const double u = X0 * iz, v = X1 * iz, fxz = Kc[0] * iz, fyz = Kc[4] * iz;
        if (!half) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double *D = R + 9 * (1 + k);
                double d[3];
                vlg_rot_b(D, b, d);
                row[2 * k] = fxz * (d[0] - u * d[2]);
                row[2 * k + 1] = fyz * (d[1] - v * d[2]);
            }
        } else {
            row[6] = fxz;  row[7] = 0.0;
            row[8] = 0.0;  row[9] = fyz;
            row[10] = -(fxz * u);
            row[11] = -(fyz * v);
            if constexpr (NA == 7) {
                row[12] = u;  row[13] = v;
            }
            if constexpr (NA == 10) {
                row[12] = u;    row[13] = 0.0;
                row[14] = 0.0;  row[15] = v;
                row[16] = 1.0;  row[17] = 0.0;
                row[18] = 0.0;  row[19] = 1.0;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                row[2 * NA + 2 * k] = fxz * (Rl[3 * k] - u * Rl[3 * k + 2]);
                row[2 * NA + 2 * k + 1] = fyz * (Rl[3 * k + 1] - v * Rl[3 * k + 2]);
            }
        }
    }
    static __device__ __forceinline__ constexpr bool jac_lane1(int col) { return col >= 3; }
};

// Radial-distortion camera (NA = BA_RAD_NA: a = [w; T; f; k1; k2], principal
// point K4[2], K4[3] fixed; vlg_project_radial).  Analytic Jacobians only: the
// context is created in that mode and cannot leave it, so the table's slots
// 1..3 always hold dR/dw_k.  The forward-difference members exist because the
// FD kernels are instantiated for every NA; no host path launches them at this
// NA, and they return the base projection.
template <>
struct cam_view<BA_RAD_NA, false> {
    static constexpr int NA = BA_RAD_NA;
    double a0[NA], c2[2], Rl[9];
    const double *R;
    __device__ __forceinline__ cam_view(const double *__restrict__ a,
                                        const double *__restrict__ K4,
                                        const double *__restrict__ rot, int j)
        : cam_view(a, K4, rot, j, j)
    {
    }
    __device__ __forceinline__ cam_view(const double *__restrict__ a,
                                        const double *__restrict__ K4,
                                        const double *__restrict__ rot, int jr, int j)
    {
#pragma unroll
        for (int c = 0; c < NA; c++) a0[c] = a[(size_t)NA * j + c];
        c2[0] = K4[4 * (size_t)j + 2];
        c2[1] = K4[4 * (size_t)j + 3];
        R = rot + 45 * (size_t)jr;
#pragma unroll
        for (int q = 0; q < 9; q++) Rl[q] = R[q];
    }
    __device__ __forceinline__ void project(const double b[3], double x[2]) const
    {
        vlg_project_radial(a0 + 6, c2, Rl, a0 + 3, b, x);
    }
    __device__ __forceinline__ void project_dcam(int, const double b[3], double x[2]) const
    {
        project(b, x);
    }
    __device__ __forceinline__ void project_col(int, const double b[3], double x[2]) const
    {
        project(b, x);
    }
    // With n = (u, v), r2, d of the projection (vlg_radial_n), g = 2 k1 +
    // 4 k2 r2:  Jn = dx/dn = f (d I + g n n'),  Jx = dx/dXc = Jn (1/z) [I | -n].
    // For a direction D of Xc, p = (D0 - u D2, D1 - v D2) / z and
    //   Jx D = (f d) p + (f g) (n'p) n.
    // A_wk = Jx (dR_k b), A_T = Jx, dx/df = d n, dx/dk1 = f r2 n, dx/dk2 =
    // f r2^2 n, B = Jx R.  Lane 0 forms the rotation columns (three 3 x 3
    // products from the table), lane 1 the other nine, which need none
    // (jac_lane1): about the same arithmetic on each.
    __device__ __forceinline__ void jac_columns(const double b[3], int half, double *row) const
    {
        double n[2], iz, r2, d;
        vlg_radial_n(a0 + 6, Rl, a0 + 3, b, n, &iz, &r2, &d);
        const double f = a0[6], u = n[0], v = n[1];
        const double g = 2.0 * a0[7] + 4.0 * (a0[8] * r2);
        const double fd = f * d, fgu = (f * g) * u, fgv = (f * g) * v;
        auto col = [&](double p0, double p1, double *o) {
            const double s = u * p0 + v * p1;
            o[0] = fd * p0 + fgu * s;
            o[1] = fd * p1 + fgv * s;
        };
        if (!half) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double *D = R + 9 * (1 + k);
                double dd[3];
                vlg_rot_b(D, b, dd);
                col(iz * (dd[0] - u * dd[2]), iz * (dd[1] - v * dd[2]), row + 2 * k);
            }
        } else {
            col(iz, 0.0, row + 6);
            col(0.0, iz, row + 8);
            col(-(iz * u), -(iz * v), row + 10);
            const double fr = f * r2, frr = fr * r2;
            row[12] = d * u;    row[13] = d * v;
            row[14] = fr * u;   row[15] = fr * v;
            row[16] = frr * u;  row[17] = frr * v;
#pragma unroll
            for (int k = 0; k < 3; k++)
                col(iz * (Rl[3 * k] - u * Rl[3 * k + 2]), iz * (Rl[3 * k + 1] - v * Rl[3 * k + 2]),
                    row + 2 * NA + 2 * k);
        }
    }
    static __device__ __forceinline__ constexpr bool jac_lane1(int col) { return col >= 3; }
};

// the point-update kernels' new projection at this model: camera j's
// parameters an (of a_new) and R(w) of its rot_new row
__device__ __forceinline__ void project_radial_new(const double an[BA_RAD_NA],
                                                   const double *__restrict__ K4,
                                                   const double *__restrict__ rot_new, int j,
                                                   const double b[3], double xh[2])
{
    double R[9];
    const double c2[2] = {K4[4 * (size_t)j + 2], K4[4 * (size_t)j + 3]};
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = rot_new[45 * (size_t)j + q];
    vlg_project_radial(an + 6, c2, R, an + 3, b, xh);
}

template <int NA>
struct cam_view<NA, true> {
    double a0[NA];
    __device__ __forceinline__ cam_view(const double *__restrict__ a, const double *, const double *,
                                        int j)
    {
#pragma unroll
        for (int c = 0; c < NA; c++) a0[c] = a[(size_t)NA * j + c];
    }
    __device__ __forceinline__ void project(const double b[3], double x[2]) const
    {
        vlg_project_proj(a0, b, x);
    }
    __device__ __forceinline__ void project_dcam(int k, const double b[3], double x[2]) const
    {
        double a1[NA];
#pragma unroll
        for (int c = 0; c < NA; c++) a1[c] = a0[c] + H_FD * ((c == k) ? 1.0 : 0.0);
        vlg_project_proj(a1, b, x);
    }
    __device__ __forceinline__ void project_col(int col, const double b[3], double x[2]) const
    {
        const bool cam = col < NA;
        double a1[NA], b1[3];
#pragma unroll
        for (int c = 0; c < NA; c++)
            a1[c] = cam ? a0[c] + H_FD * ((c == col) ? 1.0 : 0.0) : a0[c];
#pragma unroll
        for (int c = 0; c < 3; c++)
            b1[c] = cam ? b[c] : b[c] + H_FD * ((c == col - NA) ? 1.0 : 0.0);
        vlg_project_proj(a1, b1, x);
    }
    // Analytic-Jacobian mode: the quotient rule on x_ = P [b; 1], x = x_(1:2) /
    // x_(3).  With bh = [b; 1], iz = 1 / x_2, u = x_0 iz, v = x_1 iz the column
    // of P(i, j) (index i + 3 j) is (bh_j iz, 0), (0, bh_j iz), -(bh_j iz) (u, v)
    // for i = 0, 1, 2, and B_k = iz (P(0,k) - u P(2,k), P(1,k) - v P(2,k)).
    // Lane 0: columns j = 0, 1 of P; lane 1: j = 2, 3 and B.
    __device__ __forceinline__ void jac_columns(const double b[3], int half, double *row) const
    {
        const double *P = a0;
        const double x0 = P[0] * b[0] + P[3] * b[1] + P[6] * b[2] + P[9];
        const double x1 = P[1] * b[0] + P[4] * b[1] + P[7] * b[2] + P[10];
        const double x2 = P[2] * b[0] + P[5] * b[1] + P[8] * b[2] + P[11];
        const double iz = 1.0 / x2, u = x0 * iz, v = x1 * iz;
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const int j = 2 * half + jj;
            const double g = (j == 0 ? b[0] : j == 1 ? b[1] : j == 2 ? b[2] : 1.0) * iz;
            double *r = row + 6 * j;
            r[0] = g;         r[1] = 0.0;
            r[2] = 0.0;       r[3] = g;
            r[4] = -(g * u);  r[5] = -(g * v);
        }
        if (half) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                row[2 * NA + 2 * k] = iz * (P[3 * k] - u * P[3 * k + 2]);
                row[2 * NA + 2 * k + 1] = iz * (P[3 * k + 1] - v * P[3 * k + 2]);
            }
        }
    }
    static __device__ __forceinline__ constexpr bool jac_lane1(int col) { return col >= 6; }
};

// -------------------------------------------------------------------------
// rotations: R(a), R(a + h e_k) k = 0..2, R(a + 0) per camera (5 x 9)
// -------------------------------------------------------------------------
// rotation k of the table alone (k = 0: R(w); k = 1..4: as below)
__device__ __forceinline__ void rotation_k(const double w[3], int k, double *__restrict__ out)
{
    double R[9], w1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) w1[c] = k == 0 ? w[c] : w[c] + H_FD * ((c == k - 1) ? 1.0 : 0.0);
    vlg_rodrigues(R, w1);
#pragma unroll
    for (int q = 0; q < 9; q++) out[9 * k + q] = R[q];
}

// Analytic-Jacobian mode (ba_dev::jac): slot 0 R(w) as above, bit for bit;
// slots 1..3 dR/dw_k (vlg_drodrigues); slot 4 unused, zero.
__device__ __forceinline__ void rotation_k_jac(const double w[3], int k, double *__restrict__ out)
{
    if (k == 0) {
        rotation_k(w, k, out);
        return;
    }
    double D[9];
#pragma unroll
    for (int q = 0; q < 9; q++) D[q] = 0.0;
    if (k < 4) vlg_drodrigues(D, w, k - 1);
#pragma unroll
    for (int q = 0; q < 9; q++) out[9 * k + q] = D[q];
}

__device__ __forceinline__ void rotations5_jac(const double w[3], double *__restrict__ out)
{
#pragma unroll
    for (int k = 0; k < 5; k++) rotation_k_jac(w, k, out);
}

__device__ __forceinline__ void rotations5(const double w[3], double *__restrict__ out)
{
    double R[9];
    vlg_rodrigues(R, w);
#pragma unroll
    for (int q = 0; q < 9; q++) out[q] = R[q];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // derivative_camera (mex_bundle_1_XABeUVWeAeB.c:30-33): a1 = a0 + h*da,
        // da = e_k for k < 3; for k >= 3 the rotation part is a0 + h*0.
        double w1[3];
#pragma unroll
        for (int c = 0; c < 3; c++) w1[c] = w[c] + H_FD * ((c == k) ? 1.0 : 0.0);
        vlg_rodrigues(R, w1);
#pragma unroll
        for (int q = 0; q < 9; q++) out[9 * (1 + k) + q] = R[q];
    }
}

