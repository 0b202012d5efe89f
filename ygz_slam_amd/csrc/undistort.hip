// A0 -- lens undistortion in front of the pyramid: level 0 = the uploaded picture resampled into the ideal pinhole camera of the context
// (cv::initUndistortRectifyMap with R = I, then cv::remap INTER_LINEAR in its 5-bit fixed point with a constant border; k1, k2, p1, p2, k3).
// The frozen spec is tests/undist_ref.c: the map is FP64 with the spec's parentheses and no contraction, everything
// behind the map is integer, and both the map and the image are bit-identical to it.
//   k_undist_map   lane = pixel, once per ygz_hip_set_undistortion (not hot)
//   k_undistort    all requested slots in one launch; a block makes a 64 x 32 output tile (the tile of k_pyr_down), a lane 2 x 4 pixels with
//                  dword stores; the tile's source bounding box is staged in LDS (BGR -> gray once per source pixel), a box that does not fit
//                  is gathered from global memory instead.  Memory-bound.
// The map formula and the tile's body are remap_dev.h's, shared with rectify.hip: this is the rig's remap with R = I and the box reduced in
// every launch.  The host functions both files use (the source plane, the lens validation, the map download) are defined here.
// No atomics, no wait for another workgroup, no scratch, no environment switch; every address is tested against the image before it is read.
#include "remap_dev.h"
#include <string.h>
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void k_undist_map(RemapCam C, int w, int h, int32_t *__restrict__ mqx, int32_t *__restrict__ mqy)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int v = (int)(i / (unsigned)w), u = (int)(i - (unsigned)v * (unsigned)w);
    int32_t qx, qy;
    remap_q(u, v, C, w, h, qx, qy);
    mqx[i] = qx; mqy[i] = qy;
}

// src: [gridDim.z][h][w][channels] (channels 1 or 3), dst: [gridDim.z][h][w]; mqx, mqy [h][w]
__global__ __launch_bounds__(256) void k_undistort(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ mqx,
                                                   const int32_t *__restrict__ mqy, int w, int h, int channels, int border)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[RM_LDS];
    __shared__ int s_box[4][4];
    const size_t npix = (size_t)w * (size_t)h;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ox = (int)blockIdx.x * RM_TW + 4 * tx, oy0 = (int)blockIdx.y * RM_TH + ty;
    rm_i32x4 qx[2], qy[2];
    remap_load_q(mqx, mqy, w, h, ox, oy0, qx, qy);
    const RemapBox B = remap_reduce_box(qx, qy, w, h, s_box);
    remap_tile(tile, src + (size_t)blockIdx.z * npix * (size_t)channels, dst + (size_t)blockIdx.z * npix, qx, qy, B, w, h, channels, border, ox, oy0);
}

// where the source of the slots' remap is: their BGR uploads, or -- level 0 holds a gray upload and is the destination too -- the copy of their
// planes that is put aside here, on the context's current stream (the lens-only remap and the rig's share the plane)
int ygz_remap_source(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr, const uint8_t **src)
{
    const size_t npix = (size_t)ctx->lw[0] * ctx->lh[0];
    if (from_bgr) { *src = ctx->bgr + (size_t)slot_begin * npix * 3; return YGZ_OK; }
    const size_t bytes = (size_t)n_slots * npix;
    if (ctx->undist_plane_bytes < bytes) {
        if (ctx->undist_plane) { YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->undist_plane); ctx->undist_plane = nullptr; ctx->undist_plane_bytes = 0; }
        YGZ_HIPCHK(ctx, hipMalloc((void **)&ctx->undist_plane, bytes + 64));
        ctx->undist_plane_bytes = bytes;
    }
    YGZ_HIPCHK(ctx, hipMemcpyAsync(ctx->undist_plane, ctx->lvl[0] + (size_t)slot_begin * npix, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    *src = ctx->undist_plane;
    return YGZ_OK;
}

// nine finite values, positive focal lengths, a border value that is a pixel
bool ygz_lens_valid(const ygz_undistort_params &p)
{
    const double f[9] = { p.k1, p.k2, p.p1, p.p2, p.k3, p.fx, p.fy, p.cx, p.cy };
    for (double v : f) if (!isfinite(v)) return false;
    return p.fx > 0.0 && p.fy > 0.0 && p.border_value >= 0 && p.border_value <= 255;
}

// a map of the context's size to the host; dqx, dqy: the device's map, null where none is set
int ygz_remap_map_to_host(ygz_hip_ctx *ctx, const int32_t *dqx, const int32_t *dqy, int32_t *qx, int32_t *qy)
{
    if (!dqx || !dqy) return YGZ_E_STATE;
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    const size_t bytes = (size_t)ctx->lw[0] * ctx->lh[0] * sizeof(int32_t);
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qx, dqx, bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipMemcpyAsync(qy, dqy, bytes, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

// level 0 of the slots = the undistorted gray of their uploads, on the context's current stream (ygz_hip_build_pyramid_undistorted, ctx.hip)
int ygz_launch_undistort(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr)
{
    if (!ctx->undist_qx || !ctx->undist_qy) return YGZ_E_STATE;
    const int w = ctx->lw[0], h = ctx->lh[0];
    const size_t npix = (size_t)w * h;
    const uint8_t *src;
    { const int rc = ygz_remap_source(ctx, slot_begin, n_slots, from_bgr, &src); if (rc != YGZ_OK) return rc; }
    YGZ_LAUNCH(ctx, KID_UNDISTORT, k_undistort, dim3(ygz_div_up(w, RM_TW), ygz_div_up(h, RM_TH), n_slots), dim3(256), src,
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
    if (p && !ygz_lens_valid(*p)) return YGZ_E_INVALID;
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
    hipLaunchKernelGGL(k_undist_map, dim3(ygz_div_up(w * h, 256)), dim3(256), 0, ctx->stream, remap_cam(ctx, *p, nullptr), w, h, ctx->undist_qx, ctx->undist_qy);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

int ygz_hip_undistort_map(ygz_hip_ctx *ctx, int32_t *qx, int32_t *qy)
{
    YgzDeviceGuard dg_(ctx);
    if (!qx || !qy || !ctx) return YGZ_E_INVALID;
    return ygz_remap_map_to_host(ctx, ctx->undist_qx, ctx->undist_qy, qx, qy);
}

}  // extern "C"
