// Optimal proper rotation of one point set onto another from their 3 x 3 correlation matrix (Horn 1987, "Closed-form
// solution of absolute orientation using unit quaternions"): the rotation is the unit quaternion that is the eigenvector
// of the largest eigenvalue of a symmetric 4 x 4 matrix built from the correlations.  The eigenpair comes from cyclic
// Jacobi in fp64 with a fixed upper bound on the sweeps: unlike the Newton iteration on the characteristic polynomial
// (QCP) it does not care whether the largest eigenvalue is simple, so collinear, coplanar-mirrored and two-atom
// selections come out as one of their minimisers, and a non-finite input ends at once (every comparison is written
// so that NaN leaves the loop).  Host and device; one fit per thread, everything in registers (all indices are
// compile-time constants after unrolling).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HORN_HD __host__ __device__ __forceinline__
#else
#define HORN_HD inline
#endif

constexpr int kHornMaxSweeps = 16;       // 4 x 4 Jacobi reaches fp64 round-off in 5-7 sweeps; the bound is the guard
constexpr double kHornOffTol = 1.0e-34;  // sum of squared off-diagonals of the max-normalised matrix: (1e-17)^2

// One Jacobi rotation in the (P, Q) plane, P < Q, of the symmetric a (its upper triangle), accumulated into the
// eigenvector columns of v.
template <int P, int Q>
HORN_HD void horn_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (!(fabs(apq) > 1.0e-150)) return;   // zero, denormal-small or NaN: nothing to rotate
    const double d = a[Q][Q] - a[P][P];
    // t = tan of the rotation angle, the smaller root of t^2 + 2 t theta - 1 = 0 with theta = d / (2 apq)
    const double t = (d < 0.0 ? -2.0 : 2.0) * apq / (fabs(d) + sqrt(d * d + 4.0 * apq * apq));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tau = s / (1.0 + c);
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0;
    // only the upper triangle of a is kept (the lower one would be a second copy of it in registers)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            double& ekp = k < P ? a[k][P] : a[P][k];
            double& ekq = k < Q ? a[k][Q] : a[Q][k];
            const double akp = ekp, akq = ekq;
            ekp = akp - s * (akq + tau * akp);
            ekq = akq + s * (akp - tau * akq);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = vkp - s * (vkq + tau * vkp);
        v[k][Q] = vkq + s * (vkp - tau * vkq);
    }
}

// m[3 * a + b] = sum_i x_i[a] * r_i[b] over centred coordinates (x is moved, r stays).  Returns in R (row-major) the
// proper rotation maximising sum_i r_i . (R x_i) and in *lambda that maximum, so that the residual is
// sum |x|^2 + sum |r|^2 - 2 lambda.  m == 0 gives the identity; a non-finite m gives NaN everywhere.
HORN_HD void horn_fit(const double (&m)[9], double* lambda, double (&R)[9]) {
    double scale = 0.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        finite = finite && (fabs(m[i]) <= 1.0e300);   // false for NaN and Inf
        scale = fmax(scale, fabs(m[i]));
    }
    if (!finite) {
        const double bad = nan("");
        *lambda = bad;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = bad;
        return;
    }
    double qw = 1.0, qx = 0.0, qy = 0.0, qz = 0.0;
    *lambda = 0.0;
    if (scale > 0.0) {
        const double inv = 1.0 / scale;
        const double xx = m[0] * inv, xy = m[1] * inv, xz = m[2] * inv;
        const double yx = m[3] * inv, yy = m[4] * inv, yz = m[5] * inv;
        const double zx = m[6] * inv, zy = m[7] * inv, zz = m[8] * inv;
        double a[4][4] = {{xx + yy + zz, yz - zy, zx - xz, xy - yx},
                          {yz - zy, xx - yy - zz, xy + yx, zx + xz},
                          {zx - xz, xy + yx, yy - xx - zz, yz + zy},
                          {xy - yx, zx + xz, yz + zy, zz - xx - yy}};
        double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll 1
        for (int sweep = 0; sweep < kHornMaxSweeps; ++sweep) {
            const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] +
                               a[1][3] * a[1][3] + a[2][3] * a[2][3];
            if (!(off > kHornOffTol)) break;
            horn_rotate<0, 1>(a, v);
            horn_rotate<0, 2>(a, v);
            horn_rotate<0, 3>(a, v);
            horn_rotate<1, 2>(a, v);
            horn_rotate<1, 3>(a, v);
            horn_rotate<2, 3>(a, v);
        }
        // largest eigenvalue, the lowest index on a tie
        double best = a[0][0];
        qw = v[0][0]; qx = v[1][0]; qy = v[2][0]; qz = v[3][0];
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            if (a[j][j] > best) { best = a[j][j]; qw = v[0][j]; qx = v[1][j]; qy = v[2][j]; qz = v[3][j]; }
        }
        *lambda = best * scale;
        const double nrm = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
        qw *= nrm; qx *= nrm; qy *= nrm; qz *= nrm;
    }
    R[0] = qw * qw + qx * qx - qy * qy - qz * qz;
    R[1] = 2.0 * (qx * qy - qw * qz);
    R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz);
    R[4] = qw * qw - qx * qx + qy * qy - qz * qz;
    R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy);
    R[7] = 2.0 * (qy * qz + qw * qx);
    R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
}
