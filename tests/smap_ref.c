/* smap_ref.c -- restatement of stereo map-point creation, the yardstick of ygz_slam_amd/csrc/smap.hip (tests/test_smap_ref.py,
 * tests/test_gpu_smap.py).  Nothing in the reference, whose LocalMapping::CreateNewMapPoints (src/Module/LocalMapping.cpp
 * :416-495) is monocular: these are ORB-SLAM2's two creation paths, Tracking::StereoInitialization / CreateNewKeyFrame (sm_keyframe_points)
 * and LocalMapping::CreateNewMapPoints with stereo measurements (sm_create).  Test infrastructure: plain C99, single-threaded, built by
 * tests/smap_ref.py with -O2 -ffp-contract=off -fno-fast-math and never linked into the product.
 *
 * Only + - * /, sqrt and integer operations: no trigonometry.  ORB-SLAM2's stereo parallax cos(2 atan2(b / 2, d)) is the closed form
 * (d^2 - b^2 / 4) / (d^2 + b^2 / 4).  Every sum is written in one order, left to right, with the parentheses shown.  The null vector of the
 * 4 x 4 system is init_ref.c's one-sided Jacobi (ir_null_vector: pair order and stop rule stated there).
 *
 * Poses are qx qy qz qw tx ty tz, world -> camera, the quaternion of unit length (it is not normalised here); K4 = fx fy cx cy;
 * bf = fx * baseline; the scale factor of the pyramid is 2, so sigma^2 of level l is 4^l and the scale of level l is 2^l. */
#include <stddef.h>
#include "init_ref.c"

typedef struct { double baseline, chi2_mono, chi2_stereo, cos_parallax_max, ratio_factor, th_depth; int32_t min_close, pad; } sm_params;
typedef struct {
    double T1[7], T2[7];
    const double *px1, *px2, *ur1, *ur2, *depth1, *depth2;      /* [n][2], [n][2], [n] each; ur < 0: mono; depth read only where ur >= 0 */
    const int32_t *level1, *level2;
    int n;
} sm_problem;

enum { SM_OK = 0, SM_NO_METHOD = 1, SM_DEGENERATE = 2, SM_BEHIND_1 = 3, SM_BEHIND_2 = 4, SM_REPROJ_1 = 5, SM_REPROJ_2 = 6, SM_ZERO_DIST = 7, SM_SCALE = 8 };
enum { SM_NONE = 0, SM_TRIANGULATE = 1, SM_UNPROJECT_1 = 2, SM_UNPROJECT_2 = 3 };
#define SM_DMAX 1.7976931348623157e308

void sm_default_params(sm_params *p)
{
    p->baseline = 0.1; p->chi2_mono = 5.991; p->chi2_stereo = 7.8; p->cos_parallax_max = 0.9998; p->ratio_factor = 3.0; p->th_depth = 3.5;
    p->min_close = 100; p->pad = 0;
}
int sm_params_size(void) { return (int)sizeof(sm_params); }
int sm_params_offset(int field)
{
    switch (field) {
    case 0: return (int)offsetof(sm_params, baseline);
    case 1: return (int)offsetof(sm_params, chi2_mono);
    case 2: return (int)offsetof(sm_params, chi2_stereo);
    case 3: return (int)offsetof(sm_params, cos_parallax_max);
    case 4: return (int)offsetof(sm_params, ratio_factor);
    case 5: return (int)offsetof(sm_params, th_depth);
    case 6: return (int)offsetof(sm_params, min_close);
    default: return (int)offsetof(sm_params, pad);
    }
}
int sm_problem_size(void) { return (int)sizeof(sm_problem); }

/* the rotation matrix of a unit quaternion, row-major */
static void sm_rotation(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* what a pose is prepared into, once per problem: C[0..8] = R, C[9..11] = t, C[12..14] = the camera centre -R^T t */
void sm_camera(const double *T, double *C)
{
    sm_rotation(T, C);
    C[9] = T[4]; C[10] = T[5]; C[11] = T[6];
    for (int i = 0; i < 3; ++i) C[12 + i] = -((C[i] * C[9] + C[3 + i] * C[10]) + C[6 + i] * C[11]);
}

/* the stereo parallax of a point at depth d seen by a rig of baseline b: cos(2 atan2(b / 2, d)) */
double sm_cos_stereo(double d, double b)
{
    const double h = 0.5 * b, h2 = h * h, d2 = d * d;
    return (d2 - h2) / (d2 + h2);
}

static void sm_normalised(const double *px, const double *K4, double *xn)
{
    xn[0] = (px[0] - K4[2]) / K4[0]; xn[1] = (px[1] - K4[3]) / K4[1]; xn[2] = 1.0;
}

/* R^T v */
static void sm_rt_mul(const double *R, const double *v, double *o)
{
    for (int i = 0; i < 3; ++i) o[i] = (R[i] * v[0] + R[3 + i] * v[1]) + R[6 + i] * v[2];
}

/* the world point of the pixel with normalised coordinates xn at depth z: R^T (z xn - t) */
static void sm_unproject(const double *C, const double *xn, double z, double *X)
{
    double c[3];
    for (int i = 0; i < 3; ++i) c[i] = z * xn[i] - C[9 + i];
    sm_rt_mul(C, c, X);
}

/* row r of R X + t */
static double sm_cam_row(const double *C, int r, const double *X)
{
    return ((C[3 * r] * X[0] + C[3 * r + 1] * X[1]) + C[3 * r + 2] * X[2]) + C[9 + r];
}

/* the reprojection test of one camera: 1 when the point is refused */
static int sm_reproj_fails(const double *C, const double *X, double z, const double *px, double ur, int level, const double *K4, double bf,
                           const sm_params *p)
{
    const double x = sm_cam_row(C, 0, X), y = sm_cam_row(C, 1, X);
    const double u = K4[0] * (x / z) + K4[2], v = K4[1] * (y / z) + K4[3];
    const double ex = u - px[0], ey = v - px[1], s = (double)(1 << (2 * level));
    const double e2 = ex * ex + ey * ey;
    if (ur >= 0) {
        const double er = (u - bf / z) - ur;
        return e2 + er * er > p->chi2_stereo * s;
    }
    return e2 > p->chi2_mono * s;
}

static double sm_dist(const double *C, const double *X)
{
    const double a = X[0] - C[12], b = X[1] - C[13], c = X[2] - C[14];
    return sqrt((a * a + b * b) + c * c);
}

/* one pair; C1, C2 from sm_camera.  X[3] is written only for code 0 */
static void sm_pair(const double *C1, const double *C2, const double *px1, const double *px2, double ur1, double ur2, double depth1, double depth2,
                    int level1, int level2, const double *K4, const sm_params *p, int32_t *code, int32_t *method, double *Xout)
{
    double xn1[3], xn2[3], r1[3], r2[3], X[3];
    const int stereo1 = ur1 >= 0, stereo2 = ur2 >= 0;
    *code = SM_NO_METHOD; *method = SM_NONE;
    /* 1: the rays */
    sm_normalised(px1, K4, xn1); sm_normalised(px2, K4, xn2);
    sm_rt_mul(C1, xn1, r1); sm_rt_mul(C2, xn2, r2);
    const double dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
    const double n1 = sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]), n2 = sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]);
    const double cosRays = dot / (n1 * n2);
    /* 2: the stereo parallax, ORB-SLAM2's asymmetry kept (side 2 only when side 1 is not stereo) */
    double cosS1 = cosRays + 1.0, cosS2 = cosRays + 1.0;
    if (stereo1) cosS1 = sm_cos_stereo(depth1, p->baseline);
    else if (stereo2) cosS2 = sm_cos_stereo(depth2, p->baseline);
    const double cosS = cosS1 < cosS2 ? cosS1 : cosS2;
    /* 3: the method */
    if (cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || cosRays < p->cos_parallax_max)) {
        double A[16], V[16], x[4];
        *method = SM_TRIANGULATE;
        for (int c = 0; c < 4; ++c) {
            const double a0 = c < 3 ? C1[c] : C1[9], a1 = c < 3 ? C1[3 + c] : C1[10], a2 = c < 3 ? C1[6 + c] : C1[11];
            const double b0 = c < 3 ? C2[c] : C2[9], b1 = c < 3 ? C2[3 + c] : C2[10], b2 = c < 3 ? C2[6 + c] : C2[11];
            A[0 * 4 + c] = xn1[0] * a2 - a0;
            A[1 * 4 + c] = xn1[1] * a2 - a1;
            A[2 * 4 + c] = xn2[0] * b2 - b0;
            A[3 * 4 + c] = xn2[1] * b2 - b1;
        }
        ir_null_vector(A, 4, 4, V, x);
        if (x[3] == 0) { *code = SM_DEGENERATE; return; }
        for (int i = 0; i < 3; ++i) X[i] = x[i] / x[3];
        if (!(fabs(X[0]) <= SM_DMAX && fabs(X[1]) <= SM_DMAX && fabs(X[2]) <= SM_DMAX)) { *code = SM_DEGENERATE; return; }
    } else if (stereo1 && cosS1 < cosS2) {
        *method = SM_UNPROJECT_1;
        sm_unproject(C1, xn1, depth1, X);
    } else if (stereo2 && cosS2 < cosS1) {
        *method = SM_UNPROJECT_2;
        sm_unproject(C2, xn2, depth2, X);
    } else return;                                                   /* code 1 */
    /* 4: in front of both cameras (a depth that is not a number is refused with the non-positive ones) */
    const double z1 = sm_cam_row(C1, 2, X);
    if (!(z1 > 0)) { *code = SM_BEHIND_1; return; }
    const double z2 = sm_cam_row(C2, 2, X);
    if (!(z2 > 0)) { *code = SM_BEHIND_2; return; }
    /* 5: the reprojection, camera 1 then camera 2 */
    const double bf = K4[0] * p->baseline;
    if (sm_reproj_fails(C1, X, z1, px1, ur1, level1, K4, bf, p)) { *code = SM_REPROJ_1; return; }
    if (sm_reproj_fails(C2, X, z2, px2, ur2, level2, K4, bf, p)) { *code = SM_REPROJ_2; return; }
    /* 6, 7: the distances and the scale consistency */
    const double dist1 = sm_dist(C1, X), dist2 = sm_dist(C2, X);
    if (dist1 == 0 || dist2 == 0) { *code = SM_ZERO_DIST; return; }
    const double ratioDist = dist2 / dist1, ratioOctave = (double)(1 << level1) / (double)(1 << level2);
    if (ratioDist * p->ratio_factor < ratioOctave || ratioDist > ratioOctave * p->ratio_factor) { *code = SM_SCALE; return; }
    *code = SM_OK;
    Xout[0] = X[0]; Xout[1] = X[1]; Xout[2] = X[2];
}

/* (a) the pairs of one problem: code, method [n], pos_world [n][3] (zero unless code 0) */
void sm_create(const sm_problem *pb, const double *K4, const sm_params *p, int32_t *code, int32_t *method, double *pos_world)
{
    double C1[15], C2[15];
    sm_camera(pb->T1, C1); sm_camera(pb->T2, C2);
    for (int i = 0; i < pb->n; ++i) {
        const double u1 = pb->ur1[i], u2 = pb->ur2[i];
        pos_world[3 * i] = 0.0; pos_world[3 * i + 1] = 0.0; pos_world[3 * i + 2] = 0.0;
        sm_pair(C1, C2, pb->px1 + 2 * i, pb->px2 + 2 * i, u1, u2, u1 >= 0 ? pb->depth1[i] : 0.0, u2 >= 0 ? pb->depth2[i] : 0.0, pb->level1[i],
                pb->level2[i], K4, p, code + i, method + i, pos_world + 3 * i);
    }
}

/* (b) the keyframe's own points.  The features with depth > 0 are ranked by (depth, index) ascending; c counts those with depth <= th_depth;
 * the ranks 0 .. min(n_depth - 1, max(c, min_close)) are walked (ORB-SLAM2's loop breaks behind the first walked feature that is both beyond
 * th_depth and past the min_close-th); selected = walked and no point yet.  rank: the real rank of a walked feature, selected or not, and -1
 * for every other feature.  pos_world: R^T (z xn - t) of a selected feature, zero otherwise. */
void sm_keyframe_points(const double *T, const double *px, const double *depth, const uint8_t *has_point, int n, const double *K4,
                        const sm_params *p, int32_t *rank, uint8_t *selected, double *pos_world, int32_t *n_depth, int32_t *n_close)
{
    double C[15];
    int nd = 0, c = 0;
    sm_camera(T, C);
    for (int i = 0; i < n; ++i) {
        if (depth[i] > 0) { ++nd; if (depth[i] <= p->th_depth) ++c; }
    }
    const int m = c > p->min_close ? c : p->min_close, last = nd - 1 < m ? nd - 1 : m;
    for (int i = 0; i < n; ++i) {
        int r = -1;
        rank[i] = -1; selected[i] = 0;
        pos_world[3 * i] = 0.0; pos_world[3 * i + 1] = 0.0; pos_world[3 * i + 2] = 0.0;
        if (depth[i] > 0) {
            r = 0;
            for (int j = 0; j < n; ++j)
                if (depth[j] > 0 && (depth[j] < depth[i] || (depth[j] == depth[i] && j < i))) ++r;
        }
        if (r < 0 || r > last) continue;
        rank[i] = r;
        if (has_point[i]) continue;
        double xn[3];
        selected[i] = 1;
        sm_normalised(px + 2 * i, K4, xn);
        sm_unproject(C, xn, depth[i], pos_world + 3 * i);
    }
    *n_depth = nd; *n_close = c;
}
