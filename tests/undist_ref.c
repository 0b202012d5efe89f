/* The restatement of the undistortion stage (ygz_slam_amd/csrc/undistort.hip): the frozen spec of DESIGN.md section 18 in plain C99.
 * Build with gcc -O2 -ffp-contract=off -fno-fast-math (tests/undist_ref.py).  Only + - * /, rint and integer operations.
 *
 * The model is OpenCV's: initUndistortRectifyMap with R = I (k1, k2, p1, p2, k3), then remap with INTER_LINEAR in its 5-bit fixed point and a
 * constant border.  Parity with OpenCV itself is unpinned (no OpenCV where the tests run): this file is the spec. */
#include <stdint.h>
#include <math.h>

typedef struct {
    double k1, k2, p1, p2, k3;      /* Brown-Conrady coefficients of the camera that took the picture */
    double fx, fy, cx, cy;          /* its intrinsics */
    int border_value;               /* the gray value outside the picture, in [0, 255] */
} ur_params;                        /* = ygz_undistort_params */

#define UR_OUTSIDE INT32_MIN

/* the map of a w x h output image seen by the ideal camera (fx_d, fy_d, cx_d, cy_d): qx, qy [h][w], source coordinates in 1/32 pixel, or
 * UR_OUTSIDE in both */
void ur_map(int w, int h, double fx_d, double fy_d, double cx_d, double cy_d, const ur_params *p, int32_t *qx, int32_t *qy)
{
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const double x = ((double)u - cx_d) / fx_d, y = ((double)v - cy_d) / fy_d;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
            const double kr = 1.0 + ((p->k3 * r2 + p->k2) * r2 + p->k1) * r2;
            const double xd = (x * kr + p->p1 * xy2) + p->p2 * (r2 + 2.0 * x2);
            const double yd = (y * kr + p->p1 * (r2 + 2.0 * y2)) + p->p2 * xy2;
            const double mx = p->fx * xd + p->cx, my = p->fy * yd + p->cy;
            const long i = (long)v * w + u;
            if (!(mx > -2.0 && mx < (double)(w + 1) && my > -2.0 && my < (double)(h + 1))) { qx[i] = UR_OUTSIDE; qy[i] = UR_OUTSIDE; continue; }
            qx[i] = (int32_t)rint(mx * 32.0);
            qy[i] = (int32_t)rint(my * 32.0);
        }
}

/* the source camera's pixel of an output pixel, before the outside test and the fixed point (for the tests' own checks) */
void ur_map_real(int w, int h, double fx_d, double fy_d, double cx_d, double cy_d, const ur_params *p, double *mx_out, double *my_out)
{
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const double x = ((double)u - cx_d) / fx_d, y = ((double)v - cy_d) / fy_d;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
            const double kr = 1.0 + ((p->k3 * r2 + p->k2) * r2 + p->k1) * r2;
            const double xd = (x * kr + p->p1 * xy2) + p->p2 * (r2 + 2.0 * x2);
            const double yd = (y * kr + p->p1 * (r2 + 2.0 * y2)) + p->p2 * xy2;
            mx_out[(long)v * w + u] = p->fx * xd + p->cx;
            my_out[(long)v * w + u] = p->fy * yd + p->cy;
        }
}

/* (1868 B + 9617 G + 4899 R + 8192) >> 14: the project's BGR -> gray */
static int ur_gray(const uint8_t *s) { return (1868 * s[0] + 9617 * s[1] + 4899 * s[2] + 8192) >> 14; }

static int ur_tap(const uint8_t *src, int w, int h, int channels, int y, int x, int border)
{
    if (x < 0 || x >= w || y < 0 || y >= h) return border;
    const uint8_t *s = src + ((long)y * w + x) * channels;
    return channels == 3 ? ur_gray(s) : s[0];
}

/* out [h][w] from src [h][w][channels] (channels 1: gray, 3: BGR, converted per tap) through the map */
void ur_remap(int w, int h, const uint8_t *src, int channels, const int32_t *qx, const int32_t *qy, int border, uint8_t *out)
{
    for (long i = 0; i < (long)w * h; ++i) {
        if (qx[i] == UR_OUTSIDE) { out[i] = (uint8_t)border; continue; }
        const int sx = qx[i] >> 5, ax = qx[i] & 31, sy = qy[i] >> 5, ay = qy[i] & 31;
        const int t00 = ur_tap(src, w, h, channels, sy, sx, border), t01 = ur_tap(src, w, h, channels, sy, sx + 1, border);
        const int t10 = ur_tap(src, w, h, channels, sy + 1, sx, border), t11 = ur_tap(src, w, h, channels, sy + 1, sx + 1, border);
        out[i] = (uint8_t)(((32 - ax) * (32 - ay) * t00 + ax * (32 - ay) * t01 + (32 - ax) * ay * t10 + ax * ay * t11 + 512) >> 10);
    }
}

/* steps 2-3 on normalised coordinates (PinholeCamera::DistortPoint takes k3 = 0) */
void ur_distort_point(const ur_params *p, double x, double y, double *xd, double *yd)
{
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((p->k3 * r2 + p->k2) * r2 + p->k1) * r2;
    *xd = (x * kr + p->p1 * xy2) + p->p2 * (r2 + 2.0 * x2);
    *yd = (y * kr + p->p1 * (r2 + 2.0 * y2)) + p->p2 * xy2;
}

int ur_params_size(void) { return (int)sizeof(ur_params); }
