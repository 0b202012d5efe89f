// The double-precision pose arithmetic that the bit-exact solvers share: popt.hip, gba_phases.h (gba.hip, sba.hip), pgo.hip, sim3.hip,
// pnp.hip and init.hip.  Every function here is held to a CPU restatement through the kernels that call it (DESIGN.md section 39 lists
// which), so an edit changes all of them at once and has to be made in tests/*_ref.c too.  Only + - * / and sqrt, uncontracted, every sum
// in the association order written.  A pose is qx qy qz qw tx ty tz, a Sim3 adds the scale as its eighth double; matrices are row-major.
//
// Merged only where the compiler's device code for every caller stayed the parent's, instruction for instruction.  Not here, on purpose:
//   quat_to_R_d, quat_mul_d (se3_dev.h)  the same mathematical objects in Sophus/Eigen's operation order (2 q first; another association
//                                        in the product's y and z): not bit-equal to ygz_quat_rotation and ygz_quat_mul
//   lm_inv3 (ba_resident_lm.hip)         ygz_inv3's arithmetic behind a determinant guard; on shared cofactor code its kernels' code changed
//   sr_solve7 (sim3.hip)                 factor and substitutions in one; through ygz_chol_factor the pivot tests are ordered differently
//   pt_solve6 (popt.hip)                 a Cholesky that returns at the first pivot outside (0, DBL_MAX]
//   gb_inv3 (gba_phases.h)               the 3 x 3 inverse through LDL^T of a packed symmetric block
// The two retractions spell their normalisations out: a helper for q / |q| changed k_pose_opt's and k_pgo_optimize's code.
#pragma once
#include <hip/hip_runtime.h>
#pragma clang fp contract(off)

// unit quaternion -> rotation matrix in the 1 - 2 (yy + zz) form: the solvers above.  quat_to_R_d of se3_dev.h forms 2 q first and serves
// align.hip, lfuse.hip, proj.hip, strack.hip and ba_dev.h; the two differ in the last bits and are not interchangeable
__host__ __device__ __forceinline__ void ygz_quat_rotation(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__host__ __device__ __forceinline__ void ygz_mat3_vec(const double *R, const double *v, double *o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

// the Hamilton product a b, not normalised
__host__ __device__ __forceinline__ void ygz_quat_mul(const double *a, const double *b, double *q)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by - ax * bz + ay * bw + az * bx;
    q[2] = aw * bz + ax * by - ay * bx + az * bw;
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
}

// T <- Delta(d) o T with d = (omega, t): dq = normalise(omega / 2, 1), q_out = normalise(dq q), t_out = dR t + d_t
__host__ __device__ __forceinline__ void ygz_se3_retract(const double *T, const double *d, double *out)
{
    double dq[4] = { 0.5 * d[0], 0.5 * d[1], 0.5 * d[2], 1.0 }, q[4], dR[9];
    const double dn = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] = dq[k] / dn;
    ygz_quat_mul(dq, T, q);
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    ygz_quat_rotation(dq, dR);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[4 + i] = (dR[3 * i] * T[4] + dR[3 * i + 1] * T[5] + dR[3 * i + 2] * T[6]) + d[3 + i];
}

// S <- Delta(x) o S for a Sim3, x = (omega, t, sigma): the rotation as above, the scale step (2 + sigma) / (2 - sigma); 0 when |sigma| is
// not below 2
__host__ __device__ __forceinline__ int ygz_sim3_retract(const double *S, const double *x, double *out)
{
    if (!(fabs(x[6]) < 2.0)) return 0;
    double dq[4] = { 0.5 * x[0], 0.5 * x[1], 0.5 * x[2], 1.0 }, q[4], dR[9], r[3];
    const double dn = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] = dq[k] / dn;
    const double ds = (2.0 + x[6]) / (2.0 - x[6]);
    ygz_quat_mul(dq, S, q);
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    ygz_quat_rotation(dq, dR);
    ygz_mat3_vec(dR, S + 4, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[4 + k] = ds * r[k] + x[3 + k];
    out[7] = ds * S[7];
    return 1;
}

__host__ __device__ __forceinline__ void ygz_sim3_inverse(const double *S, double *Si)
{
    Si[0] = -S[0]; Si[1] = -S[1]; Si[2] = -S[2]; Si[3] = S[3];
    Si[7] = 1.0 / S[7];
    double R[9], r[3];
    ygz_quat_rotation(Si, R);
    ygz_mat3_vec(R, S + 4, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) Si[4 + k] = -(Si[7] * r[k]);
}

// adj(a) * (1 / det), det = a00 C00 + a01 C01 + a02 C02; no guard
__host__ __device__ __forceinline__ void ygz_inv3(const double *a, double *r)
{
    double C[9];
    C[0] = a[4] * a[8] - a[5] * a[7]; C[1] = a[5] * a[6] - a[3] * a[8]; C[2] = a[3] * a[7] - a[4] * a[6];
    C[3] = a[2] * a[7] - a[1] * a[8]; C[4] = a[0] * a[8] - a[2] * a[6]; C[5] = a[1] * a[6] - a[0] * a[7];
    C[6] = a[1] * a[5] - a[2] * a[4]; C[7] = a[2] * a[3] - a[0] * a[5]; C[8] = a[0] * a[4] - a[1] * a[3];
    const double inv = 1.0 / (a[0] * C[0] + a[1] * C[1] + a[2] * C[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i * 3 + j] = C[j * 3 + i] * inv;
}

// rotation matrix -> quaternion, Eigen's branches: the trace, else the largest diagonal element
__host__ __device__ __forceinline__ void ygz_quat_from_matrix(const double *m, double *q)
{
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2 * 3 + 1] - m[1 * 3 + 2]) * t;
        q[1] = (m[0 * 3 + 2] - m[2 * 3 + 0]) * t;
        q[2] = (m[1 * 3 + 0] - m[0 * 3 + 1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}

// the information weight of a pyramid level, 4^-level
__host__ __device__ __forceinline__ double ygz_level_weight(int level) { return 1.0 / (double)(1 << (2 * level)); }

// ---- dense Cholesky of an N x N block, fully unrolled: every index below is a constant, so the blocks stay in registers ----------------
// the packed upper triangle D (row by row) as a full symmetric A
template <int N> __host__ __device__ __forceinline__ void ygz_sym_unpack(const double *D, double *A)
{
    int m = 0;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b) { A[a * N + b] = D[m]; A[b * N + a] = D[m]; ++m; }
}

// A = L L^T: the lower triangle of L packed row by row into Lo; 0 when a pivot is not positive (Lo is then not to be used)
template <int N> __host__ __device__ __forceinline__ int ygz_chol_factor(const double *A, double *Lo)
{
    double L[N * N];
    int ok = 1;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = A[j * N + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * N + k] * L[j * N + k];
        ok &= d > 0;
        const double ljj = sqrt(d);
        L[j * N + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = A[i * N + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * N + k] * L[j * N + k];
            L[i * N + j] = v / ljj;
        }
    }
    int m = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Lo[m++] = L[i * N + j];
    return ok;
}

// L L^T x = b on the packed factor: forward, then backward substitution
template <int N> __host__ __device__ __forceinline__ void ygz_chol_solve_packed(const double *Lo, const double *b, double *x)
{
    double L[N * N], y[N];
    int m = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * N + j] = Lo[m++];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i * N + k] * y[k];
        y[i] = v / L[i * N + i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= L[k * N + i] * x[k];
        x[i] = v / L[i * N + i];
    }
}
