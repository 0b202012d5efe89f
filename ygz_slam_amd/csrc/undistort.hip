// A0 -- lens undistortion in front of the pyramid: level 0 = the uploaded picture resampled into the ideal pinhole camera of the context
// (cv::initUndistortRectifyMap with R = I, then cv::remap INTER_LINEAR in its 5-bit fixed point with a constant border; k1, k2, p1, p2, k3).
// The frozen spec is tests/undist_ref.c: the map is FP64 with the spec's parentheses and no contraction, everything
// behind the map is integer, and both the map and the image are bit-identical to it.
//   k_undist_map   lane = pixel, once per ygz_hip_set_undistortion (not hot)
//   k_undistort    all requested slots in one launch; a block makes a 64 x 32 output tile (the tile of k_pyr_down), a lane 2 x 4 pixels with
//                  dword stores; the tile's source bounding box is staged in LDS (BGR -> gray once per source pixel), a box that does not fit
//                  is gathered from global memory instead.  Memory-bound.
// No atomics, no wait for another workgroup, no scratch, no environment switch; every address is tested against the image before it is read.
#include "ygz_internal.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)

#define UD_OUTSIDE INT32_MIN
#define UD_TW 64
#define UD_TH 32
#define UD_LDS 16384          // bytes of staged source per tile (nine tiles per CU would fit; the registers admit six)

// the camera that took the picture (ygz_undistort_params) and the ideal one the output is seen by (the context's intrinsics as doubles)
struct UndistCam { double k1, k2, p1, p2, k3, fx, fy, cx, cy, fx_d, fy_d, cx_d, cy_d; };

// steps 1-6 of the spec for output pixel (u, v): the source position in 1/32 pixel, or UD_OUTSIDE in both
__device__ __forceinline__ void undist_q(int u, int v, const UndistCam &C, int w, int h, int32_t &qx, int32_t &qy)
{
    const double x = ((double)u - C.cx_d) / C.fx_d, y = ((double)v - C.cy_d) / C.fy_d;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((C.k3 * r2 + C.k2) * r2 + C.k1) * r2;
    const double xd = (x * kr + C.p1 * xy2) + C.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + C.p1 * (r2 + 2.0 * y2)) + C.p2 * xy2;
    const double mx = C.fx * xd + C.cx, my = C.fy * yd + C.cy;
    if (!(mx > -2.0 && mx < (double)(w + 1) && my > -2.0 && my < (double)(h + 1))) { qx = UD_OUTSIDE; qy = UD_OUTSIDE; return; }   // NaN and infinities too
    qx = (int32_t)rint(mx * 32.0);
    qy = (int32_t)rint(my * 32.0);
}

__global__ __launch_bounds__(256) void k_undist_map(UndistCam C, int w, int h, int32_t *__restrict__ mqx, int32_t *__restrict__ mqy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int v = (int)(i / (unsigned)w), u = (int)(i - (unsigned)v * (unsigned)w);
    int32_t qx, qy;
    undist_q(u, v, C, w, h, qx, qy);
    mqx[i] = qx; mqy[i] = qy;
}

// gray = (1868 B + 9617 G + 4899 R + 8192) >> 14, as image.hip
__device__ __forceinline__ uint32_t ud_gray1(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

typedef int32_t ud_i32x4 __attribute__((ext_vector_type(4)));

// src: [gridDim.z][h][w][channels] (channels 1 or 3), dst: [gridDim.z][h][w]; mqx, mqy [h][w]: the map is read (8 bytes per pixel, the same
// for every slot, so it stays in L2); computing it again per pixel -- undist_q, about 25 FP64 operations -- measured 1.5 x slower
__global__ __launch_bounds__(256) void k_undistort(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ mqx,
                                                   const int32_t *__restrict__ mqy, int w, int h, int channels, int border)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[UD_LDS];
    __shared__ int s_box[4][4];
    const size_t npix = (size_t)w * (size_t)h;
    const uint8_t *s = src + (size_t)blockIdx.z * npix * (size_t)channels;
    uint8_t *d = dst + (size_t)blockIdx.z * npix;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ox = (int)blockIdx.x * UD_TW + 4 * tx, oy0 = (int)blockIdx.y * UD_TH + ty;
    const bool w4 = (w & 3) == 0;

    // the lane's 2 x 4 map entries and the bounds of their top-left taps
    int32_t qx[2][4], qy[2][4];
    int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
#pragma unroll
        for (int k = 0; k < 4; ++k) { qx[r][k] = UD_OUTSIDE; qy[r][k] = UD_OUTSIDE; }
        if (oy < h && ox < w) {
            const size_t i = (size_t)oy * w + ox;
            if (w4) {                                              // ox % 4 == 0 and w % 4 == 0: 16-byte aligned, ox + 3 < w
                const ud_i32x4 a = *reinterpret_cast<const ud_i32x4 *>(mqx + i), b = *reinterpret_cast<const ud_i32x4 *>(mqy + i);
                qx[r][0] = a.x; qx[r][1] = a.y; qx[r][2] = a.z; qx[r][3] = a.w;
                qy[r][0] = b.x; qy[r][1] = b.y; qy[r][2] = b.z; qy[r][3] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (ox + k < w) { qx[r][k] = mqx[i + k]; qy[r][k] = mqy[i + k]; }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (qx[r][k] != UD_OUTSIDE) {
                const int sx = qx[r][k] >> 5, sy = qy[r][k] >> 5;
                bx0 = min(bx0, sx); bx1 = max(bx1, sx); by0 = min(by0, sy); by1 = max(by1, sy);
            }
    }
    // the tile's bounds: across the wavefront in registers, across the four wavefronts through 64 bytes of LDS
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, m)); bx1 = max(bx1, __shfl_xor(bx1, m));
        by0 = min(by0, __shfl_xor(by0, m)); by1 = max(by1, __shfl_xor(by1, m));
    }
    if ((threadIdx.x & 63) == 0) { int *b = s_box[threadIdx.x >> 6]; b[0] = bx0; b[1] = bx1; b[2] = by0; b[3] = by1; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) { bx0 = min(bx0, s_box[k][0]); bx1 = max(bx1, s_box[k][1]); by0 = min(by0, s_box[k][2]); by1 = max(by1, s_box[k][3]); }
    // the box of the taps that lie inside the picture (a tap is (sy, sx) .. (sy + 1, sx + 1)); x0a: its left edge on a 16-pixel boundary
    const int x0 = max(bx0, 0), x1 = (bx1 < w - 1) ? bx1 + 1 : w - 1, y0 = max(by0, 0), y1 = (by1 < h - 1) ? by1 + 1 : h - 1;
    const bool any = bx0 <= bx1 && x0 <= x1 && y0 <= y1;
    const int x0a = x0 & ~15, pitch = any ? ((x1 - x0a + 16) & ~15) : 16, rows = any ? y1 - y0 + 1 : 0;
    const bool staged = any && (long long)pitch * rows <= UD_LDS;          // uniform over the block
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
                    o[q] = ud_gray1(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u) | (ud_gray1(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u) << 8) |
                           (ud_gray1((w1 >> 16) & 255u, w1 >> 24, w2 & 255u) << 16) | (ud_gray1((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24) << 24);
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
                            o[q] |= (channels == 3 ? ud_gray1(t[0], t[1], t[2]) : (uint32_t)t[0]) << (8 * k);
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
        if (staged) return (int)tile[(y - y0) * pitch + (x - x0a)];
        const uint8_t *t = s + ((size_t)y * w + x) * (size_t)channels;
        return channels == 3 ? (int)ud_gray1(t[0], t[1], t[2]) : (int)t[0];
    };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
        if (oy >= h || ox >= w) continue;
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = (uint32_t)border;
            if (qx[r][k] != UD_OUTSIDE) {
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

static UndistCam undist_cam(const ygz_hip_ctx *ctx, const ygz_undistort_params &p)
{
    UndistCam C;
    C.k1 = p.k1; C.k2 = p.k2; C.p1 = p.p1; C.p2 = p.p2; C.k3 = p.k3; C.fx = p.fx; C.fy = p.fy; C.cx = p.cx; C.cy = p.cy;
    C.fx_d = (double)ctx->prm.fx; C.fy_d = (double)ctx->prm.fy; C.cx_d = (double)ctx->prm.cx; C.cy_d = (double)ctx->prm.cy;
    return C;
}

// level 0 of the slots = the undistorted gray of their uploads, on the context's current stream (ygz_hip_build_pyramid_undistorted, ctx.hip)
int ygz_launch_undistort(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr)
{
    if (!ctx->undist_qx || !ctx->undist_qy) return YGZ_E_STATE;
    const int w = ctx->lw[0], h = ctx->lh[0];
    const size_t npix = (size_t)w * h;
    const uint8_t *src;
    if (from_bgr) src = ctx->bgr + (size_t)slot_begin * npix * 3;
    else {
        // level 0 holds the raw upload and is the destination too: the slots' planes go aside first
        const size_t bytes = (size_t)n_slots * npix;
        if (ctx->undist_plane_bytes < bytes) {
            if (ctx->undist_plane) { YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->undist_plane); ctx->undist_plane = nullptr; ctx->undist_plane_bytes = 0; }
            YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->undist_plane, bytes + 64));
            ctx->undist_plane_bytes = bytes;
        }
        YGZ_HIPCHK(ctx, hipMemcpyAsync(ctx->undist_plane, ctx->lvl[0] + (size_t)slot_begin * npix, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        src = ctx->undist_plane;
    }
    YGZ_LAUNCH(ctx, KID_UNDISTORT, k_undistort, dim3(ygz_div_up(w, UD_TW), ygz_div_up(h, UD_TH), n_slots), dim3(256), src,
               ctx->lvl[0] + (size_t)slot_begin * npix, ctx->undist_qx, ctx->undist_qy, w, h, from_bgr ? 3 : 1,
               ctx->undist_prm.border_value);
    YGZ_HIPCHK(ctx, hipGetLastError());
    return YGZ_OK;
}

void ygz_undistort_free(ygz_hip_ctx *ctx)
{
    if (ctx->undist_qx) (void)hipFree(ctx->undist_qx);
    if (ctx->undist_qy) (void)hipFree(ctx->undist_qy);
    if (ctx->undist_plane) (void)hipFree(ctx->undist_plane);
    ctx->undist_qx = ctx->undist_qy = nullptr; ctx->undist_plane = nullptr; ctx->undist_plane_bytes = 0;
}

extern "C" {

int ygz_hip_default_undistort_params(const ygz_hip_ctx *ctx, ygz_undistort_params *p)
{
    if (!p) return YGZ_E_INVALID;
    memset(p, 0, sizeof(*p));
    if (!ctx) return YGZ_E_INVALID;
    p->fx = (double)ctx->prm.fx; p->fy = (double)ctx->prm.fy; p->cx = (double)ctx->prm.cx; p->cy = (double)ctx->prm.cy;
    return YGZ_OK;
}

int ygz_hip_set_undistortion(ygz_hip_ctx *ctx, const ygz_undistort_params *p)
{
    YgzDeviceGuard dg_(ctx);
    if (p) {
        const double f[9] = { p->k1, p->k2, p->p1, p->p2, p->k3, p->fx, p->fy, p->cx, p->cy };
        for (double v : f) if (!isfinite(v)) return YGZ_E_INVALID;
        if (!(p->fx > 0.0) || !(p->fy > 0.0) || p->border_value < 0 || p->border_value > 255) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (!p) {                                                  // drop the map (a remap in flight still reads it)
        YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->undist_qx) (void)hipFree(ctx->undist_qx);
        if (ctx->undist_qy) (void)hipFree(ctx->undist_qy);
        ctx->undist_qx = ctx->undist_qy = nullptr;
        return YGZ_OK;
    }
    const int w = ctx->lw[0], h = ctx->lh[0];
    const size_t bytes = (size_t)w * h * sizeof(int32_t) + 64;
    if (!ctx->undist_qx) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->undist_qx, bytes));
    if (!ctx->undist_qy) YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->undist_qy, bytes));
    ctx->undist_prm = *p;
    hipLaunchKernelGGL(k_undist_map, dim3(ygz_div_up(w * h, 256)), dim3(256), 0, ctx->stream, undist_cam(ctx, *p), w, h, ctx->undist_qx, ctx->undist_qy);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

int ygz_hip_undistort_map(ygz_hip_ctx *ctx, int32_t *qx, int32_t *qy)
{
    YgzDeviceGuard dg_(ctx);
    if (!qx || !qy || !ctx) return YGZ_E_INVALID;
    if (!ctx->undist_qx || !ctx->undist_qy) return YGZ_E_STATE;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    const size_t bytes = (size_t)ctx->lw[0] * ctx->lh[0] * sizeof(int32_t);
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qx, ctx->undist_qx, bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qy, ctx->undist_qy, bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

}  // extern "C"
