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
// No wait for another workgroup, no scratch, no environment switch; every address is tested against the image before it is read.
#include "ygz_internal.h"
#include "ygz_blob.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)

#define RC_OUTSIDE INT32_MIN
#define RC_TW 64
#define RC_TH 32
#define RC_LDS 16384          // bytes of staged source per tile

// the camera that took the picture, the ideal one the output is seen by (the context's intrinsics as doubles) and the rotation between them
struct RectCam { double k1, k2, p1, p2, k3, fx, fy, cx, cy, fx_d, fy_d, cx_d, cy_d, r[9]; };

// steps 1-6 of the spec for output pixel (u, v): the source position in 1/32 pixel, or RC_OUTSIDE in both
__device__ __forceinline__ void rect_q(int u, int v, const RectCam &C, int w, int h, int32_t &qx, int32_t &qy)
{
    const double x0 = ((double)u - C.cx_d) / C.fx_d, y0 = ((double)v - C.cy_d) / C.fy_d;
    const double X = (C.r[0] * x0 + C.r[3] * y0) + C.r[6], Y = (C.r[1] * x0 + C.r[4] * y0) + C.r[7], W = (C.r[2] * x0 + C.r[5] * y0) + C.r[8];
    const double x = X / W, y = Y / W;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((C.k3 * r2 + C.k2) * r2 + C.k1) * r2;
    const double xd = (x * kr + C.p1 * xy2) + C.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + C.p1 * (r2 + 2.0 * y2)) + C.p2 * xy2;
    const double mx = C.fx * xd + C.cx, my = C.fy * yd + C.cy;
    if (!(W > 0.0) || !(mx > -2.0 && mx < (double)(w + 1) && my > -2.0 && my < (double)(h + 1))) { qx = RC_OUTSIDE; qy = RC_OUTSIDE; return; }   // NaN and infinities too
    qx = (int32_t)rint(mx * 32.0);
    qy = (int32_t)rint(my * 32.0);
}

__global__ __launch_bounds__(256) void k_rect_map(RectCam C, int w, int h, int32_t *__restrict__ mqx, int32_t *__restrict__ mqy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int v = (int)(i / (unsigned)w), u = (int)(i - (unsigned)v * (unsigned)w);
    int32_t qx, qy;
    rect_q(u, v, C, w, h, qx, qy);
    mqx[i] = qx; mqy[i] = qy;
}

typedef int32_t rc_i32x4 __attribute__((ext_vector_type(4)));

// the lane's 2 x 4 map entries of tile (bx, by): lane (tx, ty) of 16 x 16 has columns 4 tx .. 4 tx + 3 of rows ty and ty + 16
__device__ __forceinline__ void rect_load_q(const int32_t *__restrict__ mqx, const int32_t *__restrict__ mqy, int w, int h, int ox, int oy0,
                                            int32_t (&qx)[2][4], int32_t (&qy)[2][4])
{
    const bool w4 = (w & 3) == 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
#pragma unroll
        for (int k = 0; k < 4; ++k) { qx[r][k] = RC_OUTSIDE; qy[r][k] = RC_OUTSIDE; }
        if (oy < h && ox < w) {
            const size_t i = (size_t)oy * w + ox;
            if (w4) {                                              // ox % 4 == 0 and w % 4 == 0: 16-byte aligned, ox + 3 < w
                const rc_i32x4 a = *reinterpret_cast<const rc_i32x4 *>(mqx + i), b = *reinterpret_cast<const rc_i32x4 *>(mqy + i);
                qx[r][0] = a.x; qx[r][1] = a.y; qx[r][2] = a.z; qx[r][3] = a.w;
                qy[r][0] = b.x; qy[r][1] = b.y; qy[r][2] = b.z; qy[r][3] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (ox + k < w) { qx[r][k] = mqx[i + k]; qy[r][k] = mqy[i + k]; }
            }
        }
    }
}

// the box of a tile: the source pixels its in-picture taps touch (a tap is (sy, sx) .. (sy + 1, sx + 1)).  x0a: the left edge on a 16-pixel
// boundary; pitch: its width in whole groups of 16; rows > 0: staged in LDS (pitch * rows <= RC_LDS), rows < 0: -rows rows that do not fit
// (gathered from global memory), rows == 0: no tap inside the picture
struct RectBox { int x0a, y0, pitch, rows; };

// all 256 lanes: the box of the tile whose map entries the lanes hold (s_box: 64 bytes of LDS; ends behind a barrier)
__device__ __forceinline__ RectBox rect_reduce_box(const int32_t (&qx)[2][4], const int32_t (&qy)[2][4], int w, int h, int (*s_box)[4])
{
    int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (qx[r][k] != RC_OUTSIDE) {
                const int sx = qx[r][k] >> 5, sy = qy[r][k] >> 5;
                bx0 = min(bx0, sx); bx1 = max(bx1, sx); by0 = min(by0, sy); by1 = max(by1, sy);
            }
    // across the wavefront in registers, across the four wavefronts through 64 bytes of LDS
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, m)); bx1 = max(bx1, __shfl_xor(bx1, m));
        by0 = min(by0, __shfl_xor(by0, m)); by1 = max(by1, __shfl_xor(by1, m));
    }
    if ((threadIdx.x & 63) == 0) { int *b = s_box[threadIdx.x >> 6]; b[0] = bx0; b[1] = bx1; b[2] = by0; b[3] = by1; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) { bx0 = min(bx0, s_box[k][0]); bx1 = max(bx1, s_box[k][1]); by0 = min(by0, s_box[k][2]); by1 = max(by1, s_box[k][3]); }
    const int x0 = max(bx0, 0), x1 = (bx1 < w - 1) ? bx1 + 1 : w - 1, y0 = max(by0, 0), y1 = (by1 < h - 1) ? by1 + 1 : h - 1;
    const bool any = bx0 <= bx1 && x0 <= x1 && y0 <= y1;
    RectBox B;
    B.x0a = any ? (x0 & ~15) : 0; B.y0 = any ? y0 : 0;
    B.pitch = any ? ((x1 - B.x0a + 16) & ~15) : 16;
    const int rows = any ? y1 - y0 + 1 : 0;
    B.rows = (long long)B.pitch * rows <= RC_LDS ? rows : -rows;
    return B;
}

__global__ __launch_bounds__(256) void k_rect_boxes(const int32_t *__restrict__ mqx, const int32_t *__restrict__ mqy, int w, int h, RectBox *__restrict__ boxes)
{
    __shared__ int s_box[4][4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int32_t qx[2][4], qy[2][4];
    rect_load_q(mqx, mqy, w, h, (int)blockIdx.x * RC_TW + 4 * tx, (int)blockIdx.y * RC_TH + ty, qx, qy);
    const RectBox B = rect_reduce_box(qx, qy, w, h, s_box);
    if (threadIdx.x == 0) boxes[blockIdx.y * gridDim.x + blockIdx.x] = B;
}

// gray = (1868 B + 9617 G + 4899 R + 8192) >> 14, as image.hip
__device__ __forceinline__ uint32_t rc_gray1(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// the two cameras of the rig, by value: a block selects its camera's pointers and border value with its list entry
struct RectTab { const int32_t *qx[YGZ_RECT_CAMERAS], *qy[YGZ_RECT_CAMERAS]; const RectBox *box[YGZ_RECT_CAMERAS]; int border[YGZ_RECT_CAMERAS]; };

// src: [n][h][w][channels] (channels 1 or 3), dst: [n][h][w], both from the first requested slot; list [gridDim.z]: 2 * (slot - slot_begin) +
// camera, in camera order, so that one map (2.4 MB at VGA, an XCD's L2 holds 4 MiB) is live at a time
__global__ __launch_bounds__(256) void k_rectify(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, RectTab T, const int32_t *__restrict__ list,
                                                 int w, int h, int channels)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[RC_LDS];
    const int entry = list[blockIdx.z], cam = entry & 1, slot = entry >> 1;
    const int32_t *mqx = cam ? T.qx[1] : T.qx[0], *mqy = cam ? T.qy[1] : T.qy[0];
    const int border = cam ? T.border[1] : T.border[0];
    const size_t npix = (size_t)w * (size_t)h;
    const uint8_t *s = src + (size_t)slot * npix * (size_t)channels;
    uint8_t *d = dst + (size_t)slot * npix;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ox = (int)blockIdx.x * RC_TW + 4 * tx, oy0 = (int)blockIdx.y * RC_TH + ty;
    const bool w4 = (w & 3) == 0;

    int32_t qx[2][4], qy[2][4];
    rect_load_q(mqx, mqy, w, h, ox, oy0, qx, qy);

    const RectBox B = (cam ? T.box[1] : T.box[0])[blockIdx.y * gridDim.x + blockIdx.x];
    const int x0a = B.x0a, y0 = B.y0, pitch = B.pitch, rows = B.rows;
    const bool staged = rows > 0;                                            // uniform over the block
    if (staged) {
        const int groups = pitch >> 4, items = rows * groups;
        const bool w16 = (w & 15) == 0;                                      // then every group lies inside its row and is 16-byte aligned
        for (int i = (int)threadIdx.x; i < items; i += 256) {
            const int r = i / groups, c = (i - r * groups) * 16;
            const int y = y0 + r, x = x0a + c;
            const uint8_t *p = s + ((size_t)y * w + x) * (size_t)channels;
            uint32_t o[4];
            if (w16 && channels == 3) {
                const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1], c4 = reinterpret_cast<const uint4 *>(p)[2];
                const uint32_t v[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c4.x, c4.y, c4.z, c4.w };
#pragma unroll
                for (int q = 0; q < 4; ++q) {                                // 4 pixels = 12 bytes = 3 words
                    const uint32_t w0 = v[3 * q], w1 = v[3 * q + 1], w2 = v[3 * q + 2];
                    o[q] = rc_gray1(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u) | (rc_gray1(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u) << 8) |
                           (rc_gray1((w1 >> 16) & 255u, w1 >> 24, w2 & 255u) << 16) | (rc_gray1((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24) << 24);
                }
            } else if (w16) {
                const uint4 a = *reinterpret_cast<const uint4 *>(p);
                o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[q] = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = 4 * q + k;
                        if (x + j < w) {                                     // the rest of the group is never read back
                            const uint8_t *t = p + (size_t)j * channels;
                            o[q] |= (channels == 3 ? rc_gray1(t[0], t[1], t[2]) : (uint32_t)t[0]) << (8 * k);
                        }
                    }
                }
            }
            *reinterpret_cast<uint4 *>(&tile[r * pitch + c]) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }
    // a tap outside the picture is the border value; one inside lies in the staged box by construction of the box
    auto tap = [&](int y, int x) -> int {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return border;
        if (staged) return (int)tile[((y - y0) * pitch + (x - x0a)) & (RC_LDS - 1)];
        const uint8_t *t = s + ((size_t)y * w + x) * (size_t)channels;
        return channels == 3 ? (int)rc_gray1(t[0], t[1], t[2]) : (int)t[0];
    };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
        if (oy >= h || ox >= w) continue;
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = (uint32_t)border;
            if (qx[r][k] != RC_OUTSIDE) {
                const int sx = qx[r][k] >> 5, ax = qx[r][k] & 31, sy = qy[r][k] >> 5, ay = qy[r][k] & 31;
                const int t00 = tap(sy, sx), t01 = tap(sy, sx + 1), t10 = tap(sy + 1, sx), t11 = tap(sy + 1, sx + 1);
                px[k] = (uint32_t)(((32 - ax) * (32 - ay) * t00 + ax * (32 - ay) * t01 + (32 - ax) * ay * t10 + ax * ay * t11 + 512) >> 10);
            }
        }
        uint8_t *o = d + (size_t)oy * w + ox;
        if (w4) *reinterpret_cast<uint32_t *>(o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (ox + k < w) o[k] = (uint8_t)px[k];
        }
    }
}

static RectCam rect_cam(const ygz_hip_ctx *ctx, const ygz_rectify_params &p)
{
    RectCam C;
    const ygz_undistort_params &l = p.lens;
    C.k1 = l.k1; C.k2 = l.k2; C.p1 = l.p1; C.p2 = l.p2; C.k3 = l.k3; C.fx = l.fx; C.fy = l.fy; C.cx = l.cx; C.cy = l.cy;
    C.fx_d = (double)ctx->prm.fx; C.fy_d = (double)ctx->prm.fy; C.cx_d = (double)ctx->prm.cx; C.cy_d = (double)ctx->prm.cy;
    for (int i = 0; i < 9; ++i) C.r[i] = p.R[i];
    return C;
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
    if (from_bgr) src = ctx->bgr + (size_t)slot_begin * npix * 3;
    else {
        // level 0 holds the raw upload and is the destination too: the slots' planes go aside first (the plane of the lens-only remap)
        const size_t bytes = (size_t)n_slots * npix;
        if (ctx->undist_plane_bytes < bytes) {
            if (ctx->undist_plane) { YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->undist_plane); ctx->undist_plane = nullptr; ctx->undist_plane_bytes = 0; }
            YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->undist_plane, bytes + 64));
            ctx->undist_plane_bytes = bytes;
        }
        YGZ_HIPCHK(ctx, hipMemcpyAsync(ctx->undist_plane, ctx->lvl[0] + (size_t)slot_begin * npix, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        src = ctx->undist_plane;
    }
    RectTab T;
    for (int cam = 0; cam < YGZ_RECT_CAMERAS; ++cam) {
        T.qx[cam] = ctx->rect_qx[cam]; T.qy[cam] = ctx->rect_qy[cam]; T.box[cam] = (const RectBox *)ctx->rect_box[cam];
        T.border[cam] = ctx->rect_prm[cam].lens.border_value;
    }
    YGZ_LAUNCH(ctx, KID_RECTIFY, k_rectify, dim3(ygz_div_up(w, RC_TW), ygz_div_up(h, RC_TH), n_slots), dim3(256), src,
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
        const ygz_undistort_params &l = p->lens;
        const double f[9] = { l.k1, l.k2, l.p1, l.p2, l.k3, l.fx, l.fy, l.cx, l.cy };
        for (double v : f) if (!rect_finite(v)) return YGZ_E_INVALID;
        if (!(l.fx > 0.0) || !(l.fy > 0.0) || l.border_value < 0 || l.border_value > 255) return YGZ_E_INVALID;
        if (!rect_is_rotation(p->R)) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (!p) {                                                  // drop the map and the table (a remap in flight still reads them)
        YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        rect_drop(ctx, camera);
        return YGZ_OK;
    }
    const int w = ctx->lw[0], h = ctx->lh[0], tiles_x = ygz_div_up(w, RC_TW), tiles_y = ygz_div_up(h, RC_TH);
    const size_t bytes = (size_t)w * h * sizeof(int32_t) + 64;
    if (ctx->rect_qx[camera]) YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // a remap in flight reads the map that is rewritten
    if (!ctx->rect_qx[camera]) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->rect_qx[camera], bytes));
    if (!ctx->rect_qy[camera]) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->rect_qy[camera], bytes));
    if (!ctx->rect_box[camera]) YGZ_HIPCHK(ctx, hipMalloc(&ctx->rect_box[camera], (size_t)tiles_x * tiles_y * sizeof(RectBox)));
    ctx->rect_prm[camera] = *p;
    hipLaunchKernelGGL(k_rect_map, dim3(ygz_div_up(w * h, 256)), dim3(256), 0, ctx->stream, rect_cam(ctx, *p), w, h, ctx->rect_qx[camera], ctx->rect_qy[camera]);
    hipLaunchKernelGGL(k_rect_boxes, dim3(tiles_x, tiles_y), dim3(256), 0, ctx->stream, ctx->rect_qx[camera], ctx->rect_qy[camera], w, h,
                       (RectBox *)ctx->rect_box[camera]);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

int ygz_hip_rectify_map(ygz_hip_ctx *ctx, int camera, int32_t *qx, int32_t *qy)
{
    YgzDeviceGuard dg_(ctx);
    if (camera < 0 || camera >= YGZ_RECT_CAMERAS || !qx || !qy || !ctx) return YGZ_E_INVALID;
    if (!ctx->rect_qx[camera] || !ctx->rect_qy[camera]) return YGZ_E_STATE;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    const size_t bytes = (size_t)ctx->lw[0] * ctx->lh[0] * sizeof(int32_t);
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qx, ctx->rect_qx[camera], bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qy, ctx->rect_qy[camera], bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

}  // extern "C"
