// A0b -- stereo rectification in front of the pyramid: level 0 of a slot = the raw picture of its rig camera resampled into the context's ideal
// camera turned by that camera's rectifying rotation (cv::stereoRectify for R1 and R2, cv::initUndistortRectifyMap with R = R1 or R2, then
// cv::remap INTER_LINEAR in its 5-bit fixed point with a constant border).  The frozen spec is tests/rect_ref.c: the
// rotations and the maps are FP64 with the spec's parentheses and no contraction, everything behind the maps is integer, and the rotations, the
// maps and the images are bit-identical to it.
//   ygz_hip_stereo_rectify   host code, no device
//   k_rect_map     lane = pixel, once per ygz_hip_set_rectification (not hot)
//   k_rect_boxes   block = 64 x 32 output tile, once per map: the source bounding box of the tile's in-picture taps
//   k_rectify      all requested slots of both cameras in one launch, walked in camera order; a block makes one tile of one slot, a lane 2 x 4
//                  pixels with dword stores; the tile's box comes from the table and is staged in LDS (BGR -> gray once per source pixel), a box
//                  that does not fit is gathered from global memory instead.  Reading the box instead of reducing it in every launch is
//                  1.4 x; still bound by the per-pixel LDS reads, not by HBM.
// The map formula, the box and the tile's body are remap_dev.h's, shared with the lens-only remap, which is this one with R = I; the source
// plane, the lens validation and the map download are the host functions of that file.
// No wait for another workgroup, no scratch, no environment switch; every address is tested against the image before it is read.
#include "remap_dev.h"
#include "ygz_blob.h"
#include <string.h>
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void k_rect_map(RemapCam C, int w, int h, int32_t *__restrict__ mqx, int32_t *__restrict__ mqy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int v = (int)(i / (unsigned)w), u = (int)(i - (unsigned)v * (unsigned)w);
    int32_t qx, qy;
    remap_q(u, v, C, w, h, qx, qy);
    mqx[i] = qx; mqy[i] = qy;
}

__global__ __launch_bounds__(256) void k_rect_boxes(const int32_t *__restrict__ mqx, const int32_t *__restrict__ mqy, int w, int h, RemapBox *__restrict__ boxes)
{
    __shared__ int s_box[4][4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    rm_i32x4 qx[2], qy[2];
    remap_load_q(mqx, mqy, w, h, (int)blockIdx.x * RM_TW + 4 * tx, (int)blockIdx.y * RM_TH + ty, qx, qy);
    const RemapBox B = remap_reduce_box(qx, qy, w, h, s_box);
    if (threadIdx.x == 0) boxes[blockIdx.y * gridDim.x + blockIdx.x] = B;
}

// the two cameras of the rig, by value: a block selects its camera's pointers and border value with its list entry
struct RectTab { const int32_t *qx[YGZ_RECT_CAMERAS], *qy[YGZ_RECT_CAMERAS]; const RemapBox *box[YGZ_RECT_CAMERAS]; int border[YGZ_RECT_CAMERAS]; };

// src: [n][h][w][channels] (channels 1 or 3), dst: [n][h][w], both from the first requested slot; list [gridDim.z]: 2 * (slot - slot_begin) +
// camera, in camera order, so that one map (2.4 MB at VGA, an XCD's L2 holds 4 MiB) is live at a time
__global__ __launch_bounds__(256) void k_rectify(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, RectTab T, const int32_t *__restrict__ list,
                                                 int w, int h, int channels)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[RM_LDS];
    const int entry = list[blockIdx.z], cam = entry & 1, slot = entry >> 1;
    const int32_t *mqx = cam ? T.qx[1] : T.qx[0], *mqy = cam ? T.qy[1] : T.qy[0];
    const int border = cam ? T.border[1] : T.border[0];
    const size_t npix = (size_t)w * (size_t)h;
    const uint8_t *s = src + (size_t)slot * npix * (size_t)channels;
    uint8_t *d = dst + (size_t)slot * npix;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ox = (int)blockIdx.x * RM_TW + 4 * tx, oy0 = (int)blockIdx.y * RM_TH + ty;
    rm_i32x4 qx[2], qy[2];
    remap_load_q(mqx, mqy, w, h, ox, oy0, qx, qy);
    const RemapBox B = (cam ? T.box[1] : T.box[0])[blockIdx.y * gridDim.x + blockIdx.x];
    remap_tile(tile, s, d, qx, qy, B, w, h, channels, border, ox, oy0);
}

// level 0 of the slots = their uploads through their cameras' maps, on the context's current stream (ygz_hip_build_pyramid_rectified, ctx.hip,
// which has checked the table's values and that every named camera has a map)
int ygz_launch_rectify(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr, const uint8_t *camera_of_slot)
{
    const int w = ctx->lw[0], h = ctx->lh[0];
    const size_t npix = (size_t)w * h;
    // the slots in camera order (stable), through one packed block
    YgzBlobLayout lay;
    const size_t o_list = lay.add_n<int32_t>((size_t)n_slots);
    YgzBlob b;
    { const int rc = ygz_blob_open(ctx, SCR_RECT, lay.end, lay.end, &b); if (rc != YGZ_OK) return rc; }
    int32_t *list = ygz_at<int32_t>(b.host, o_list);
    int n = 0;
    for (int cam = 0; cam < YGZ_RECT_CAMERAS; ++cam)
        for (int i = 0; i < n_slots; ++i) if (camera_of_slot[i] == cam) list[n++] = 2 * i + cam;
    if (n != n_slots) return YGZ_E_INVALID;
    { const int rc = ygz_blob_upload(ctx, b, lay.end); if (rc != YGZ_OK) return rc; }
    const uint8_t *src;
    { const int rc = ygz_remap_source(ctx, slot_begin, n_slots, from_bgr, &src); if (rc != YGZ_OK) return rc; }
    RectTab T;
    for (int cam = 0; cam < YGZ_RECT_CAMERAS; ++cam) {
        T.qx[cam] = ctx->rect_qx[cam]; T.qy[cam] = ctx->rect_qy[cam]; T.box[cam] = (const RemapBox *)ctx->rect_box[cam];
        T.border[cam] = ctx->rect_prm[cam].lens.border_value;
    }
    YGZ_LAUNCH(ctx, KID_RECTIFY, k_rectify, dim3(ygz_div_up(w, RM_TW), ygz_div_up(h, RM_TH), n_slots), dim3(256), src,
               ctx->lvl[0] + (size_t)slot_begin * npix, T, ygz_at<const int32_t>(b.dev, o_list), w, h, from_bgr ? 3 : 1);
    YGZ_HIPCHK(ctx, hipGetLastError());
    return YGZ_OK;
}

static void rect_drop(ygz_hip_ctx *ctx, int cam)
{
    if (ctx->rect_qx[cam]) (void)hipFree(ctx->rect_qx[cam]);
    if (ctx->rect_qy[cam]) (void)hipFree(ctx->rect_qy[cam]);
    if (ctx->rect_box[cam]) (void)hipFree(ctx->rect_box[cam]);
    ctx->rect_qx[cam] = ctx->rect_qy[cam] = nullptr; ctx->rect_box[cam] = nullptr;
}

void ygz_rectify_free(ygz_hip_ctx *ctx)
{
    for (int cam = 0; cam < YGZ_RECT_CAMERAS; ++cam) rect_drop(ctx, cam);
}

// ---- the rotations of the rig: tests/rect_ref.c rr_stereo_rectify with its parentheses (host code)
static bool rect_finite(double v) { return v - v == 0.0; }

static bool rect_is_rotation(const double *R)
{
    for (int i = 0; i < 9; ++i) if (!rect_finite(R[i])) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (i == j ? 1.0 : 0.0);
            if (!(d <= 1e-6 && d >= -1e-6)) return false;
        }
    const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;
}

static void rect_quat_matrix(double a, double b, double c, double d, double *M)
{
    M[0] = 1.0 - 2.0 * (c * c + d * d); M[1] = 2.0 * (b * c - a * d);       M[2] = 2.0 * (b * d + a * c);
    M[3] = 2.0 * (b * c + a * d);       M[4] = 1.0 - 2.0 * (b * b + d * d); M[5] = 2.0 * (c * d - a * b);
    M[6] = 2.0 * (b * d - a * c);       M[7] = 2.0 * (c * d + a * b);       M[8] = 1.0 - 2.0 * (b * b + c * c);
}

static void rect_mul33(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

extern "C" {

int ygz_hip_stereo_rectify(const double R[9], const double T[3], double R1[9], double R2[9], double *baseline)
{
    if (!R || !T || !R1 || !R2 || !baseline) return YGZ_E_INVALID;
    for (int i = 0; i < 3; ++i) if (!rect_finite(T[i])) return YGZ_E_INVALID;
    if (!rect_is_rotation(R)) return YGZ_E_INVALID;
    // 1: the quaternion of R, Shepperd's method with the largest of the four candidates
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
    if (!(w > 0.5)) return YGZ_E_INVALID;                    // the cameras are 120 degrees or more apart
    // 2: the half rotation
    const double hw = 1.0 + w, nh = sqrt((hw * hw + x * x) + (y * y + z * z));
    double Rh[9], rr[9], rrT[9];
    rect_quat_matrix(hw / nh, x / nh, y / nh, z / nh, Rh);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { rr[3 * i + j] = Rh[3 * j + i]; rrT[3 * i + j] = Rh[3 * i + j]; }
    // 3: the baseline in the half-turned frame
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = (rr[3 * i] * T[0] + rr[3 * i + 1] * T[1]) + rr[3 * i + 2] * T[2];
    const double b = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (!(b > 0.0) || !rect_finite(b)) return YGZ_E_INVALID;
    const double a0 = t[0] < 0.0 ? -t[0] : t[0], a1 = t[1] < 0.0 ? -t[1] : t[1], a2 = t[2] < 0.0 ? -t[2] : t[2];
    if (!(t[0] < 0.0) || a0 < (a1 > a2 ? a1 : a2)) return YGZ_E_INVALID;      // the second camera is not to the right
    const double e0 = t[0] / b, e1 = t[1] / b, e2 = t[2] / b;
    // 4: the rotation that takes e to uu = (-1, 0, 0): v = e x uu = (0, -e2, e1), c = e . uu = -e0
    const double vy = -e2, vz = e1, k = 1.0 / (1.0 + (-e0));
    double wR[9];
    wR[0] = 1.0 + (-(vy * vy + vz * vz)) * k; wR[1] = -vz;                    wR[2] = vy;
    wR[3] = vz;                               wR[4] = 1.0 + (-(vz * vz)) * k; wR[5] = (vy * vz) * k;
    wR[6] = -vy;                              wR[7] = (vy * vz) * k;          wR[8] = 1.0 + (-(vy * vy)) * k;
    // 5
    double o1[9], o2[9];
    rect_mul33(wR, rrT, o1);
    rect_mul33(wR, rr, o2);
    for (int i = 0; i < 9; ++i) { R1[i] = o1[i]; R2[i] = o2[i]; }
    *baseline = b;
    return YGZ_OK;
}

int ygz_hip_default_rectify_params(const ygz_hip_ctx *ctx, ygz_rectify_params *p)
{
    if (!p) return YGZ_E_INVALID;
    memset(p, 0, sizeof(*p));
    if (!ctx) return YGZ_E_INVALID;
    p->lens.fx = (double)ctx->prm.fx; p->lens.fy = (double)ctx->prm.fy; p->lens.cx = (double)ctx->prm.cx; p->lens.cy = (double)ctx->prm.cy;
    p->R[0] = p->R[4] = p->R[8] = 1.0;
    return YGZ_OK;
}

int ygz_hip_set_rectification(ygz_hip_ctx *ctx, int camera, const ygz_rectify_params *p)
{
    YgzDeviceGuard dg_(ctx);
    if (camera < 0 || camera >= YGZ_RECT_CAMERAS) return YGZ_E_INVALID;
    if (p) {
        if (!ygz_lens_valid(p->lens) || !rect_is_rotation(p->R)) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (!p) {                                                  // drop the map and the table (a remap in flight still reads them)
        YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        rect_drop(ctx, camera);
        return YGZ_OK;
    }
    const int w = ctx->lw[0], h = ctx->lh[0], tiles_x = ygz_div_up(w, RM_TW), tiles_y = ygz_div_up(h, RM_TH);
    const size_t bytes = (size_t)w * h * sizeof(int32_t) + 64;
    if (ctx->rect_qx[camera]) YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // a remap in flight reads the map that is rewritten
    if (!ctx->rect_qx[camera]) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->rect_qx[camera], bytes));
    if (!ctx->rect_qy[camera]) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->rect_qy[camera], bytes));
    if (!ctx->rect_box[camera]) YGZ_HIPCHK(ctx, hipMalloc(&ctx->rect_box[camera], (size_t)tiles_x * tiles_y * sizeof(RemapBox)));
    ctx->rect_prm[camera] = *p;
    hipLaunchKernelGGL(k_rect_map, dim3(ygz_div_up(w * h, 256)), dim3(256), 0, ctx->stream, remap_cam(ctx, p->lens, p->R), w, h, ctx->rect_qx[camera], ctx->rect_qy[camera]);
    hipLaunchKernelGGL(k_rect_boxes, dim3(tiles_x, tiles_y), dim3(256), 0, ctx->stream, ctx->rect_qx[camera], ctx->rect_qy[camera], w, h,
                       (RemapBox *)ctx->rect_box[camera]);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

int ygz_hip_rectify_map(ygz_hip_ctx *ctx, int camera, int32_t *qx, int32_t *qy)
{
    YgzDeviceGuard dg_(ctx);
    if (camera < 0 || camera >= YGZ_RECT_CAMERAS || !qx || !qy || !ctx) return YGZ_E_INVALID;
    return ygz_remap_map_to_host(ctx, ctx->rect_qx[camera], ctx->rect_qy[camera], qx, qy);
}

}  // extern "C"
