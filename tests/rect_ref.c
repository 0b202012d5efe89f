/* The restatement of the stereo rectification (ygz_slam_amd/csrc/rectify.hip): the frozen spec of DESIGN.md section 23 in plain C99.
 * Build with gcc -O2 -ffp-contract=off -fno-fast-math (tests/rect_ref.py).  Only + - * /, sqrt, rint and integer operations.
 *
 * The model is OpenCV's: stereoRectify (Bouguet's method: both cameras turned by half of their relative rotation, then both turned so that
 * the baseline lies along -x) without its trigonometry, then initUndistortRectifyMap with R = R1 or R2 on the lens model of tests/undist_ref.c.
 * The remap behind the map is ur_remap of that file, not restated here.  Parity with OpenCV itself is unpinned: this file is the spec. */
#include <stdint.h>
#include <stddef.h>
#include <math.h>

typedef struct {
    double k1, k2, p1, p2, k3;
    double fx, fy, cx, cy;
    int border_value;
} rr_lens;                          /* = ur_params = ygz_undistort_params */

typedef struct {
    rr_lens lens;                   /* the camera that took the picture */
    double R[9];                    /* row-major: R1 or R2 of rr_stereo_rectify */
} rr_params;                        /* = ygz_rectify_params */

#define RR_OUTSIDE INT32_MIN
#define RR_OK 0
#define RR_INVALID 1

/* 0 when R (row-major) is a rotation: finite, max |R R^T - I| <= 1e-6, det > 0 */
int rr_rotation_check(const double *R)
{
    for (int i = 0; i < 9; ++i) if (!(R[i] - R[i] == 0.0)) return RR_INVALID;          /* NaN and infinities */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (i == j ? 1.0 : 0.0);
            if (!(d <= 1e-6 && d >= -1e-6)) return RR_INVALID;
        }
    const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(det > 0.0)) return RR_INVALID;
    return RR_OK;
}

/* the matrix (row-major) of the unit quaternion (a, b, c, d) */
static void rr_quat_matrix(double a, double b, double c, double d, double *M)
{
    M[0] = 1.0 - 2.0 * (c * c + d * d); M[1] = 2.0 * (b * c - a * d);       M[2] = 2.0 * (b * d + a * c);
    M[3] = 2.0 * (b * c + a * d);       M[4] = 1.0 - 2.0 * (b * b + d * d); M[5] = 2.0 * (c * d - a * b);
    M[6] = 2.0 * (b * d - a * c);       M[7] = 2.0 * (c * d + a * b);       M[8] = 1.0 - 2.0 * (b * b + c * c);
}

static void rr_mul33(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

/* X_right = R X_left + T.  R1, R2: the rotations that take the left and the right camera's rays into the common rectified frame, in which the
 * right camera sits at (baseline, 0, 0) of the left one.  RR_INVALID as the spec lists */
int rr_stereo_rectify(const double *R, const double *T, double *R1, double *R2, double *baseline)
{
    for (int i = 0; i < 3; ++i) if (!(T[i] - T[i] == 0.0)) return RR_INVALID;
    if (rr_rotation_check(R) != RR_OK) return RR_INVALID;
    /* 1: the quaternion of R, Shepperd's method with the largest of the four candidates */
    const double tr = (R[0] + R[4]) + R[8];
    const double c0 = 1.0 + tr, c1 = (1.0 + 2.0 * R[0]) - tr, c2 = (1.0 + 2.0 * R[4]) - tr, c3 = (1.0 + 2.0 * R[8]) - tr;
    double w, x, y, z;
    if (c0 >= c1 && c0 >= c2 && c0 >= c3) {
        const double s = sqrt(c0), f = 0.5 / s;
        w = 0.5 * s; x = (R[7] - R[5]) * f; y = (R[2] - R[6]) * f; z = (R[3] - R[1]) * f;
    } else if (c1 >= c2 && c1 >= c3) {
        const double s = sqrt(c1), f = 0.5 / s;
        x = 0.5 * s; w = (R[7] - R[5]) * f; y = (R[1] + R[3]) * f; z = (R[2] + R[6]) * f;
    } else if (c2 >= c3) {
        const double s = sqrt(c2), f = 0.5 / s;
        y = 0.5 * s; w = (R[2] - R[6]) * f; x = (R[1] + R[3]) * f; z = (R[5] + R[7]) * f;
    } else {
        const double s = sqrt(c3), f = 0.5 / s;
        z = 0.5 * s; w = (R[3] - R[1]) * f; x = (R[2] + R[6]) * f; y = (R[5] + R[7]) * f;
    }
    const double nq = sqrt((w * w + x * x) + (y * y + z * z));
    w = w / nq; x = x / nq; y = y / nq; z = z / nq;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    if (!(w > 0.5)) return RR_INVALID;                       /* the cameras are 120 degrees or more apart */
    /* 2: the half rotation */
    const double hw = 1.0 + w, nh = sqrt((hw * hw + x * x) + (y * y + z * z));
    double Rh[9], rr[9], rrT[9];
    rr_quat_matrix(hw / nh, x / nh, y / nh, z / nh, Rh);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { rr[3 * i + j] = Rh[3 * j + i]; rrT[3 * i + j] = Rh[3 * i + j]; }
    /* 3: the baseline in the half-turned frame */
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = (rr[3 * i] * T[0] + rr[3 * i + 1] * T[1]) + rr[3 * i + 2] * T[2];
    const double b = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (!(b > 0.0) || !(b - b == 0.0)) return RR_INVALID;
    const double a0 = t[0] < 0.0 ? -t[0] : t[0], a1 = t[1] < 0.0 ? -t[1] : t[1], a2 = t[2] < 0.0 ? -t[2] : t[2];
    if (!(t[0] < 0.0) || a0 < (a1 > a2 ? a1 : a2)) return RR_INVALID;      /* the second camera is not to the right */
    const double e0 = t[0] / b, e1 = t[1] / b, e2 = t[2] / b;
    /* 4: the rotation that takes e to uu = (-1, 0, 0): v = e x uu = (0, -e2, e1), c = e . uu = -e0 */
    const double vy = -e2, vz = e1, k = 1.0 / (1.0 + (-e0));
    double wR[9];
    wR[0] = 1.0 + (-(vy * vy + vz * vz)) * k; wR[1] = -vz;                    wR[2] = vy;
    wR[3] = vz;                               wR[4] = 1.0 + (-(vz * vz)) * k; wR[5] = (vy * vz) * k;
    wR[6] = -vy;                              wR[7] = (vy * vz) * k;          wR[8] = 1.0 + (-(vy * vy)) * k;
    /* 5 */
    rr_mul33(wR, rrT, R1);
    rr_mul33(wR, rr, R2);
    *baseline = b;
    return RR_OK;
}

/* steps 1-6 for one output pixel: the source camera's pixel; returns 0 when W <= 0 (or NaN) */
static int rr_pixel(int u, int v, double fx_d, double fy_d, double cx_d, double cy_d, const rr_params *p, double *mx, double *my)
{
    const double *r = p->R;
    const rr_lens *l = &p->lens;
    const double x0 = ((double)u - cx_d) / fx_d, y0 = ((double)v - cy_d) / fy_d;
    const double X = (r[0] * x0 + r[3] * y0) + r[6], Y = (r[1] * x0 + r[4] * y0) + r[7], W = (r[2] * x0 + r[5] * y0) + r[8];
    const double x = X / W, y = Y / W;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((l->k3 * r2 + l->k2) * r2 + l->k1) * r2;
    const double xd = (x * kr + l->p1 * xy2) + l->p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + l->p1 * (r2 + 2.0 * y2)) + l->p2 * xy2;
    *mx = l->fx * xd + l->cx; *my = l->fy * yd + l->cy;
    return W > 0.0;
}

/* the map of camera k: qx, qy [h][w], source coordinates in 1/32 pixel, or RR_OUTSIDE in both */
void rr_map(int w, int h, double fx_d, double fy_d, double cx_d, double cy_d, const rr_params *p, int32_t *qx, int32_t *qy)
{
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            double mx, my;
            const int front = rr_pixel(u, v, fx_d, fy_d, cx_d, cy_d, p, &mx, &my);
            const long i = (long)v * w + u;
            if (!front || !(mx > -2.0 && mx < (double)(w + 1) && my > -2.0 && my < (double)(h + 1))) { qx[i] = RR_OUTSIDE; qy[i] = RR_OUTSIDE; continue; }
            qx[i] = (int32_t)rint(mx * 32.0);
            qy[i] = (int32_t)rint(my * 32.0);
        }
}

/* the source pixel before the outside test and the fixed point (for the tests' own checks); front [h][w]: W > 0 */
void rr_map_real(int w, int h, double fx_d, double fy_d, double cx_d, double cy_d, const rr_params *p, double *mx_out, double *my_out, uint8_t *front)
{
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const long i = (long)v * w + u;
            front[i] = (uint8_t)rr_pixel(u, v, fx_d, fy_d, cx_d, cy_d, p, &mx_out[i], &my_out[i]);
        }
}

int rr_params_size(void) { return (int)sizeof(rr_params); }
int rr_params_offset_R(void) { return (int)offsetof(rr_params, R); }
