/*
 * vlg_math.h -- deterministic fp64 math of the gfx950 kernels (product code;
 * the CPU oracle restates the same reference formulas independently with the
 * host libm and never includes this file).
 *
 * Why this file exists
 * --------------------
 * The reference builds every Jacobian by forward differences with h = 1e-10
 * (toolbox/bundle/mex_bundle_1_XABeUVWeAeB.c:23,39-40,52,68-69).  A one-ulp
 * difference in a projection is amplified by 1/h, so the device projection has
 * to be bit-identical to the reference arithmetic: the rotations use glibc's
 * own sin / cos algorithm (vlg_libm.h, equal to the host libm bit for bit),
 * every expression keeps the reference's evaluation order, the kernels are
 * compiled with -ffp-contract=off, and '/' and sqrt are IEEE (HIP f64 '/' and
 * sqrt are correctly rounded).
 *
 * Contents
 *   vlg_rodrigues           VLFeat vl_rodrigues (R only), SURVEY.md App. B,
 *                           called from toolbox/bundle/reproject_point.h:44
 *   vlg_calib, vlg_project  toolbox/bundle/reproject_point.h:16-57 with the
 *                           rotation supplied by the caller (so a kernel can
 *                           hoist the per-camera Rodrigues out of the
 *                           per-observation loop without changing a bit)
 *   vlg_project_proj        reproject_projective_point of
 *                           toolbox/bundle/mex_bundle_proj_1_XABeUVWeAeB.c:13-32
 *   vlg_project_radial      the radial-distortion camera (num_a = 9: one focal
 *                           length, two radial coefficients; not part of the
 *                           reference)
 *   vlg_drodrigues          dR/dw_k of the exponential map (analytic-Jacobian
 *                           mode; not part of the reference)
 *   vlg_loss                robust loss of one observation (Huber, Cauchy)
 *   vlg_fd_quot             (x1 - x0) / h without a division, bit-identical
 *   vlg_pinv3               3x3 pseudo-inverse of the damped point blocks
 *
 * Every expression keeps the reference's evaluation order.
 * Include from C99, C++ or HIP.
 */
#ifndef VLG_MATH_H
#define VLG_MATH_H

#if defined(__HIPCC__)
#define VLG_HD __host__ __device__ static inline
#else
#define VLG_HD static inline
#endif

#include <stdint.h>
#include <string.h>
#include <math.h>

#include "vlg_libm.h"

/* sin / cos of the rotations: glibc's algorithm (vlg_libm.h), bit-identical to
 * the host libm that VLFeat's vl_rodrigues -- and the oracle -- call */
#define VLG_SIN vlg_lm_sin
#define VLG_COS vlg_lm_cos

/* ---- Rodrigues: rotation vector -> R (3x3, column major R[i + 3*j]) --------
 * VLFeat vl_rodrigues (not vendored; spec recovered in SURVEY.md App. B):
 * theta < 1e-6 gives exactly I, which makes the finite-difference rotation
 * Jacobian exactly zero for cameras with |w| < ~1e-6 (App. A Q2).            */
VLG_HD void vlg_rodrigues(double R[9], const double om[3])
{
    const double small = 1e-6;
    double th = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    double x, y, z, xx, xy, xz, yy, yz, zz, sth, cth, mcth;
    if (th < small) {
        R[0] = 1.0; R[3] = 0.0; R[6] = 0.0;
        R[1] = 0.0; R[4] = 1.0; R[7] = 0.0;
        R[2] = 0.0; R[5] = 0.0; R[8] = 1.0;
        return;
    }
    x = om[0] / th;
    y = om[1] / th;
    z = om[2] / th;
    xx = x * x; xy = x * y; xz = x * z;
    yy = y * y; yz = y * z; zz = z * z;
    sth = VLG_SIN(th);
    cth = VLG_COS(th);
    mcth = 1.0 - cth;
    R[0] = 1 - mcth * (yy + zz);
    R[1] = sth * z + mcth * xy;
    R[2] = -sth * y + mcth * xz;
    R[3] = -sth * z + mcth * xy;
    R[4] = 1 - mcth * (zz + xx);
    R[5] = sth * x + mcth * yz;
    R[6] = sth * y + mcth * xz;
    R[7] = -sth * x + mcth * yz;
    R[8] = 1 - mcth * (xx + yy);
}

/* ---- dR/dw_k of the exponential map (analytic-Jacobian mode) ---------------
 * R = I + A K + B K^2, K = [w]x, A = sin th / th, B = (1 - cos th) / th^2 and
 * K^2 = w w' - th^2 I, so with a1 = A'(th) / th, b1 = B'(th) / th
 *   dR/dw_k = w_k a1 K + A G_k + w_k b1 K^2 + B (e_k w' + w e_k' - 2 w_k I),
 * G_k = [e_k]x.  Below VLG_DROD_SERIES the four coefficients are their Taylor
 * series in th^2: the closed forms a1 = (th cos th - sin th) / th^3 and
 * b1 = (th sin th - 2 (1 - cos th)) / th^4 cancel to a relative error of about
 * 3 u / th^2 and 12 u / th^2 (48 u at the switch-over, th = 0.5), while the
 * series' first dropped term there is below 1e-17 of the sum.  th < 1e-6:
 * vlg_rodrigues returns exactly I; the derivative is the limit G_k all the
 * same, so a camera at w = 0 can rotate.  Column major dR[i + 3*j].          */
#define VLG_DROD_SERIES 0.5
VLG_HD void vlg_drodrigues(double dR[9], const double om[3], int k)
{
    const double x = om[0], y = om[1], z = om[2];
    const double t2 = x * x + y * y + z * z;
    const double th = sqrt(t2);
    const double wk = k == 0 ? x : (k == 1 ? y : z);
    double A, B, a1, b1;
    if (th < 1e-6) {
        A = 1.0; B = 0.0; a1 = 0.0; b1 = 0.0;
    } else if (th < VLG_DROD_SERIES) {
        /* sum_n (-1)^n t2^n / (2n+1)!, / (2n+2)!, and their th-derivatives / th */
        A = 1.0 + t2 * (-1.0 / 6 + t2 * (1.0 / 120 + t2 * (-1.0 / 5040 + t2 * (1.0 / 362880 +
            t2 * (-1.0 / 39916800 + t2 * (1.0 / 6227020800.0 + t2 * (-1.0 / 1307674368000.0)))))));
        B = 0.5 + t2 * (-1.0 / 24 + t2 * (1.0 / 720 + t2 * (-1.0 / 40320 + t2 * (1.0 / 3628800 +
            t2 * (-1.0 / 479001600 + t2 * (1.0 / 87178291200.0 + t2 * (-1.0 / 20922789888000.0)))))));
        a1 = -1.0 / 3 + t2 * (1.0 / 30 + t2 * (-1.0 / 840 + t2 * (1.0 / 45360 +
             t2 * (-1.0 / 3991680 + t2 * (1.0 / 518918400 + t2 * (-1.0 / 93405312000.0))))));
        b1 = -1.0 / 12 + t2 * (1.0 / 180 + t2 * (-1.0 / 6720 + t2 * (1.0 / 453600 +
             t2 * (-1.0 / 47900160 + t2 * (1.0 / 7264857600.0 + t2 * (-1.0 / 1494484992000.0))))));
    } else {
        const double s = VLG_SIN(th), c = VLG_COS(th), mc = 1.0 - c;
        A = s / th;
        B = mc / t2;
        a1 = (th * c - s) / (t2 * th);
        b1 = (th * s - 2.0 * mc) / (t2 * t2);
    }
    {
        const double p = wk * a1, q = wk * b1, d = -2.0 * wk * B - q * t2;
        /* w_k a1 K + w_k b1 (w w' - th^2 I) + B (e_k w' + w e_k' - 2 w_k I) */
        dR[0] = q * (x * x) + d;
        dR[4] = q * (y * y) + d;
        dR[8] = q * (z * z) + d;
        dR[1] = q * (x * y) + p * z;
        dR[3] = q * (x * y) - p * z;
        dR[2] = q * (x * z) - p * y;
        dR[6] = q * (x * z) + p * y;
        dR[5] = q * (y * z) + p * x;
        dR[7] = q * (y * z) - p * x;
        /* + A G_k and the e_k rows / columns of B (e_k w' + w e_k') */
        if (k == 0) {
            dR[0] += 2.0 * (B * x); dR[1] += B * y; dR[3] += B * y; dR[2] += B * z; dR[6] += B * z;
            dR[5] += A; dR[7] -= A;
        } else if (k == 1) {
            dR[4] += 2.0 * (B * y); dR[1] += B * x; dR[3] += B * x; dR[5] += B * z; dR[7] += B * z;
            dR[6] += A; dR[2] -= A;
        } else {
            dR[8] += 2.0 * (B * z); dR[2] += B * x; dR[6] += B * x; dR[5] += B * y; dR[7] += B * y;
            dR[1] += A; dR[3] -= A;
        }
    }
}

/* ---- calibration override: reproject_point.h:29-41 ----------------------
 * Kc[9] starts as the 3x3 built from the 4-vector [fx fy cx cy]
 * (mex_bundle_1_XABeUVWeAeB.c:186-188); num_variableK 1 uses a[6] for both
 * focal lengths (App. A Q13), num_variableK 4 uses a[6..9].                 */
VLG_HD void vlg_calib(double Kc[9], const double K4[4], const double *a, int nvk)
{
    Kc[0] = K4[0]; Kc[3] = 0.0;   Kc[6] = K4[2];
    Kc[1] = 0.0;   Kc[4] = K4[1]; Kc[7] = K4[3];
    Kc[2] = 0.0;   Kc[5] = 0.0;   Kc[8] = 1.0;
    if (nvk == 1) {
        Kc[0] = a[6];
        Kc[4] = a[6];
    } else if (nvk == 4) {
        Kc[0] = a[6];
        Kc[4] = a[7];
        Kc[6] = a[8];
        Kc[7] = a[9];
    }
}

/* ---- projection: reproject_point.h:46-56, rotation given -----------------
 * x = dehom(Kc * (R*b + t)), every sum left-to-right as written there.      */
/* The same expression in two steps, so a kernel can share the rotated point
 * between projections that differ only in t: S = R*b without t (the first
 * three terms of each left-to-right row sum), then x = dehom(Kc * (S + t)).
 * vlg_project(Kc, R, t, b) == vlg_project_s(Kc, S, t) for S = vlg_rot_b(R, b)
 * bit for bit: C evaluates ((R0 b0 + R3 b1) + R6 b2) + t0 in that order. */
VLG_HD void vlg_rot_b(const double R[9], const double b[3], double S[3])
{
    S[0] = R[0] * b[0] + R[3] * b[1] + R[6] * b[2];
    S[1] = R[1] * b[0] + R[4] * b[1] + R[7] * b[2];
    S[2] = R[2] * b[0] + R[5] * b[1] + R[8] * b[2];
}

/* the homogeneous image point Kc * (S + t) before the division */
VLG_HD void vlg_project_h(const double Kc[9], const double S[3], const double t[3], double xn[3])
{
    double Rb0 = S[0] + t[0];
    double Rb1 = S[1] + t[1];
    double Rb2 = S[2] + t[2];
    xn[0] = Kc[0] * Rb0 + Kc[3] * Rb1 + Kc[6] * Rb2;
    xn[1] = Kc[1] * Rb0 + Kc[4] * Rb1 + Kc[7] * Rb2;
    xn[2] = Kc[2] * Rb0 + Kc[5] * Rb1 + Kc[8] * Rb2;
}

VLG_HD void vlg_project_s(const double Kc[9], const double S[3], const double t[3], double x[2])
{
    double xn[3];
    vlg_project_h(Kc, S, t, xn);
    x[0] = xn[0] / xn[2];
    x[1] = xn[1] / xn[2];
}

VLG_HD void vlg_project(const double Kc[9], const double R[9], const double t[3],
                        const double b[3], double x[2])
{
    double S[3];
    vlg_rot_b(R, b, S);
    vlg_project_s(Kc, S, t, x);
}

/* Projective camera (a = P(:), 3 x 4 column major, num_a = 12):
 * x_ = P [b; 1], x = x_(1:2) / x_(3), each row summed left to right
 * (mex_bundle_proj_1_XABeUVWeAeB.c:13-32, identical in
 * mex_bundle_proj_3_db_new.c:13-31). */
VLG_HD void vlg_project_proj(const double P[12], const double b[3], double x[2])
{
    double x0 = P[0] * b[0] + P[3] * b[1] + P[6] * b[2] + P[9];
    double x1 = P[1] * b[0] + P[4] * b[1] + P[7] * b[2] + P[10];
    double x2 = P[2] * b[0] + P[5] * b[1] + P[8] * b[2] + P[11];
    x[0] = x0 / x2;
    x[1] = x1 / x2;
}

/* ---- radial-distortion camera (num_a = 9; not part of the reference) --------
 * a = [w; T; f; k1; k2], the principal point c = (cx, cy) fixed:
 *   Xc = R b + T,  n = (Xc0, Xc1) / Xc2,  r2 = n'n,
 *   d = (1 + k1 r2) + (k2 r2) r2,  x = f (d n) + c
 * (the Bundler / BAL model with a positive focal length and depth).  The one
 * projection of the model: every kernel that projects calls it, and
 * vlg_radial_n gives the Jacobian's closed form the same n, r2 and d bit for
 * bit.  k = a + 6 = [f; k1; k2].                                              */
VLG_HD void vlg_radial_n(const double k[3], const double R[9], const double t[3],
                         const double b[3], double n[2], double *iz, double *r2, double *d)
{
    double S[3];
    vlg_rot_b(R, b, S);
    {
        const double X0 = S[0] + t[0], X1 = S[1] + t[1], X2 = S[2] + t[2];
        const double u = X0 / X2, v = X1 / X2;
        const double q = u * u + v * v;
        n[0] = u;
        n[1] = v;
        *iz = 1.0 / X2;
        *r2 = q;
        *d = (1.0 + k[1] * q) + (k[2] * q) * q;
    }
}

VLG_HD void vlg_project_radial(const double k[3], const double c[2], const double R[9],
                               const double t[3], const double b[3], double x[2])
{
    double n[2], iz, r2, d;
    vlg_radial_n(k, R, t, b, n, &iz, &r2, &d);
    x[0] = k[0] * (d * n[0]) + c[0];
    x[1] = k[0] * (d * n[1]) + c[1];
}

/* ---- robust loss of one observation (first-order IRLS) ----
 * s = e0^2 + e1^2 in pixels^2, c the scale in pixels.  rho(s) is the
 * observation's cost, sqrtw = sqrt(rho'(s)) the factor of its Jacobian rows and
 * residual.
 *   1 Huber   rho = s (s <= c^2), else 2 c sqrt(s) - c^2;  w = 1, else c / sqrt(s)
 *   2 Cauchy  rho = c^2 log1p(s / c^2);                     w = 1 / (1 + s / c^2)
 * The inlier branch of Huber returns s and 1.0 themselves: with every s below
 * c^2 a pass computes the bits of the plain one.                               */
VLG_HD void vlg_loss(int kind, double c, double s, double *rho, double *sqrtw)
{
    const double c2 = c * c;
    if (kind == 1) {
        if (s <= c2) {
            *rho = s;
            *sqrtw = 1.0;
        } else {
            const double r = sqrt(s);
            *rho = 2.0 * c * r - c2;
            *sqrtw = sqrt(c / r);
        }
    } else if (kind == 2) {
        const double q = s / c2;
        *rho = c2 * log1p(q);
        *sqrtw = sqrt(1.0 / (1.0 + q));
    } else {
        *rho = s;
        *sqrtw = 1.0;
    }
}

/* the observation's cost is the plain term s = e0 e0 + e1 e1 itself (no loss, a
 * Huber inlier): the batched one-block passes, whose plain cost adds e0 e0 and
 * e1 e1 one after the other (MATLAB's flat e(:)'e(:)), add such a term that way
 * under a loss too, so Huber with every s below c^2 keeps the plain bits */
VLG_HD int vlg_loss_plain(int kind, double c, double s)
{
    return kind == 1 ? s <= c * c : kind != 2;
}

/* Finite-difference step of the reference (mex_bundle_1_XABeUVWeAeB.c:23,52). */
#define VLG_FD_H 1e-10

/* (x1 - x0) / h of the forward differences (mex_bundle_1 :39-40, 68-69),
 * correctly rounded without a division.  Markstein's theorem (IBM J. R&D 34,
 * 1990; Cornea-Hasegan, Golliver, Markstein, ARITH-14 1999): if y is within
 * half an ulp of 1/h and q is within one ulp of d/h, the remainder
 * r = d - q h is exact (one FMA) and RN(q + r y) = RN(d/h).  Here
 * y = RN(1/h) and y h = 1 + e1 with |e1| <= 2^-54 (checked exactly in
 * tests/test_oracle.py::test_fd_quotient), so q = RN(d y) is within one ulp
 * of d/h.  Both theorems need d and q h away from the subnormal range; tiny
 * |d| (including 0, whose sign the remainder step would lose) and non-finite
 * d take the plain division.  The device uses this (3 fp64 ops instead of
 * ~10 + a quarter-rate reciprocal); the oracle keeps '/' as the reference
 * writes it, and the stage-1 parity tests compare the two bit for bit. */
#define VLG_FD_RH (1.0 / VLG_FD_H)
VLG_HD double vlg_fd_quot(double d)
{
    const double ad = fabs(d);
    if (!(ad >= 0x1p-900 && ad <= 0x1p900)) return d / VLG_FD_H;
    const double q = d * VLG_FD_RH;
    const double r = fma(-q, VLG_FD_H, d);
    return fma(r, VLG_FD_RH, q);
}

/* ---- 3x3 symmetric pseudo-inverse ------------------------------------------
 * The reference inverts every damped point block with MATLAB pinv
 * (bundle_euclid.m:180).  Here: adjugate / determinant for a well-conditioned
 * block, an all-zero block maps to zero (pinv(0) = 0, App. A Q8), and a
 * numerically singular block goes through a cyclic-Jacobi eigen pseudo-inverse
 * with MATLAB's tolerance max(size)*eps(sigma_max).  The same function runs on
 * the device and in the oracle's "device-formula" mode; the oracle's "pinv"
 * mode uses an SVD instead, and the tests bound the gap between the two.     */
VLG_HD double vlg_eps_of(double x)
{
    int e;
    if (!(x > 0.0))
        return 4.9406564584124654e-324;
    (void)frexp(x, &e); /* x = f * 2^e, f in [0.5,1) */
    return ldexp(1.0, e - 53);
}

VLG_HD void vlg_pinv3_jacobi(const double M[9], double P[9])
{
    double a[3][3], q[3][3], d[3], smax, tol;
    int i, j, k, sweep;
    for (i = 0; i < 3; i++)
        for (j = 0; j < 3; j++) {
            a[i][j] = 0.5 * (M[i + 3 * j] + M[j + 3 * i]);
            q[i][j] = (i == j) ? 1.0 : 0.0;
        }
    for (sweep = 0; sweep < 32; sweep++) {
        double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off == 0.0)
            break;
        for (i = 0; i < 2; i++)
            for (j = i + 1; j < 3; j++) {
                double apq = a[i][j], theta, t, c, s;
                if (apq == 0.0)
                    continue;
                theta = (a[j][j] - a[i][i]) / (2.0 * apq);
                t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                c = 1.0 / sqrt(t * t + 1.0);
                s = t * c;
                for (k = 0; k < 3; k++) { /* A <- A J */
                    double akp = a[k][i], akq = a[k][j];
                    a[k][i] = c * akp - s * akq;
                    a[k][j] = s * akp + c * akq;
                }
                for (k = 0; k < 3; k++) { /* A <- J^T A */
                    double apk = a[i][k], aqk = a[j][k];
                    a[i][k] = c * apk - s * aqk;
                    a[j][k] = s * apk + c * aqk;
                }
                for (k = 0; k < 3; k++) { /* Q <- Q J */
                    double qkp = q[k][i], qkq = q[k][j];
                    q[k][i] = c * qkp - s * qkq;
                    q[k][j] = s * qkp + c * qkq;
                }
            }
    }
    smax = 0.0;
    for (i = 0; i < 3; i++) {
        d[i] = a[i][i];
        if (fabs(d[i]) > smax)
            smax = fabs(d[i]);
    }
    tol = 3.0 * vlg_eps_of(smax);
    for (i = 0; i < 9; i++)
        P[i] = 0.0;
    for (k = 0; k < 3; k++) {
        double inv;
        if (!(fabs(d[k]) > tol))
            continue;
        inv = 1.0 / d[k];
        for (i = 0; i < 3; i++)
            for (j = 0; j < 3; j++)
                P[i + 3 * j] += q[i][k] * q[j][k] * inv;
    }
}

VLG_HD void vlg_pinv3(const double M[9], double P[9])
{
    double m00 = M[0], m10 = M[1], m20 = M[2];
    double m01 = M[3], m11 = M[4], m21 = M[5];
    double m02 = M[6], m12 = M[7], m22 = M[8];
    double c00 = m11 * m22 - m12 * m21;
    double c01 = m12 * m20 - m10 * m22;
    double c02 = m10 * m21 - m11 * m20;
    double c10 = m02 * m21 - m01 * m22;
    double c11 = m00 * m22 - m02 * m20;
    double c12 = m01 * m20 - m00 * m21;
    double c20 = m01 * m12 - m02 * m11;
    double c21 = m02 * m10 - m00 * m12;
    double c22 = m00 * m11 - m01 * m10;
    double det = m00 * c00 + m01 * c01 + m02 * c02;
    double s = 0.0, r;
    int i;
    for (i = 0; i < 9; i++)
        if (fabs(M[i]) > s)
            s = fabs(M[i]);
    if (s == 0.0) {
        for (i = 0; i < 9; i++)
            P[i] = 0.0;
        return;
    }
    if (!(fabs(det) > 1e-12 * s * s * s)) {
        vlg_pinv3_jacobi(M, P);
        return;
    }
    r = 1.0 / det;
    P[0] = c00 * r; P[3] = c10 * r; P[6] = c20 * r;
    P[1] = c01 * r; P[4] = c11 * r; P[7] = c21 * r;
    P[2] = c02 * r; P[5] = c12 * r; P[8] = c22 * r;
}

#endif /* VLG_MATH_H */
