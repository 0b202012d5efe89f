// The level-0 remap, once: cv::initUndistortRectifyMap, then cv::remap INTER_LINEAR in its 5-bit fixed point with a constant border.  The kernels
// of undistort.hip (lens only) and rectify.hip (a rig camera behind its rectifying rotation) are launches around these device functions; the
// frozen specs are tests/undist_ref.c and tests/rect_ref.c (DESIGN.md sections 18 and 23).  The map is FP64 with the specs' parentheses and no
// contraction, everything behind the map is integer.
//
// The lens-only map is the rig map with R = I, bit for bit, so remap_q is the one function that makes a map integer:
//   x0 and y0 are finite: the ideal camera's intrinsics are finite single-precision values with fx_d, fy_d > 0, so neither quotient overflows a double;
//   X = (1 x0 + 0 y0) + 0 is x0 up to the sign of a zero, and Y is y0 likewise;
//   W = (0 x0 + 0 y0) + 1 is exactly 1, so x0 / W is x0 and W > 0 holds;
//   the sign of a zero changes no comparison, and on its way through the lens polynomial to (int32_t)rint(mx * 32.0) it can at most make a
//   zero of the other sign, which is the same integer.
// No wait for another workgroup, no scratch, no environment switch; every address is tested against the image before it is read.
#pragma once
#include "ygz_internal.h"
#include <limits.h>
#include <math.h>
#pragma clang fp contract(off)

#define RM_OUTSIDE INT32_MIN
#define RM_TW 64
#define RM_TH 32
#define RM_LDS 16384          // bytes of staged source per tile (nine tiles per CU would fit; the registers admit six or seven)

// the camera that took the picture, the ideal one the output is seen by (the context's intrinsics as doubles) and the rotation between them
struct RemapCam { double k1, k2, p1, p2, k3, fx, fy, cx, cy, fx_d, fy_d, cx_d, cy_d, r[9]; };

// R: row-major 3 x 3, or null for the identity (the lens-only map)
static inline RemapCam remap_cam(const ygz_hip_ctx *ctx, const ygz_undistort_params &l, const double *R)
{
    RemapCam C;
    C.k1 = l.k1; C.k2 = l.k2; C.p1 = l.p1; C.p2 = l.p2; C.k3 = l.k3; C.fx = l.fx; C.fy = l.fy; C.cx = l.cx; C.cy = l.cy;
    C.fx_d = (double)ctx->prm.fx; C.fy_d = (double)ctx->prm.fy; C.cx_d = (double)ctx->prm.cx; C.cy_d = (double)ctx->prm.cy;
    for (int i = 0; i < 9; ++i) C.r[i] = R ? R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    return C;
}

// steps 1-6 of the specs for output pixel (u, v): the source position in 1/32 pixel, or RM_OUTSIDE in both
__device__ __forceinline__ void remap_q(int u, int v, const RemapCam &C, int w, int h, int32_t &qx, int32_t &qy)
{
    const double x0 = ((double)u - C.cx_d) / C.fx_d, y0 = ((double)v - C.cy_d) / C.fy_d;
    const double X = (C.r[0] * x0 + C.r[3] * y0) + C.r[6], Y = (C.r[1] * x0 + C.r[4] * y0) + C.r[7], W = (C.r[2] * x0 + C.r[5] * y0) + C.r[8];
    const double x = X / W, y = Y / W;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double kr = 1.0 + ((C.k3 * r2 + C.k2) * r2 + C.k1) * r2;
    const double xd = (x * kr + C.p1 * xy2) + C.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + C.p1 * (r2 + 2.0 * y2)) + C.p2 * xy2;
    const double mx = C.fx * xd + C.cx, my = C.fy * yd + C.cy;
    if (!(W > 0.0) || !(mx > -2.0 && mx < (double)(w + 1) && my > -2.0 && my < (double)(h + 1))) { qx = RM_OUTSIDE; qy = RM_OUTSIDE; return; }   // NaN and infinities too
    qx = (int32_t)rint(mx * 32.0);
    qy = (int32_t)rint(my * 32.0);
}

// gray = (1868 B + 9617 G + 4899 R + 8192) >> 14, as image.hip
__device__ __forceinline__ uint32_t remap_gray1(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

typedef int32_t rm_i32x4 __attribute__((ext_vector_type(4)));

// the lane's 2 x 4 map entries of a 64 x 32 tile: lane (tx, ty) of 16 x 16 has columns ox = 4 tx .. 4 tx + 3 of rows oy0 = ty and ty + 16.  The map is
// read (8 bytes per pixel, the same for every slot, so it stays in L2); computing it again per pixel -- remap_q, about 25 FP64 operations --
// measured 1.5 x slower.  A row's four entries stay the vector they are loaded as: as sixteen separate integers handed
// from function to function, the second row's load landed in spare registers and was copied behind a wait in front of the staging loop (4 % of k_rectify)
__device__ __forceinline__ void remap_load_q(const int32_t *__restrict__ mqx, const int32_t *__restrict__ mqy, int w, int h, int ox, int oy0,
                                             rm_i32x4 (&qx)[2], rm_i32x4 (&qy)[2])
{
    const bool w4 = (w & 3) == 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
#pragma unroll
        for (int k = 0; k < 4; ++k) { qx[r][k] = RM_OUTSIDE; qy[r][k] = RM_OUTSIDE; }
        if (oy < h && ox < w) {
            const size_t i = (size_t)oy * w + ox;
            if (w4) {                                              // ox % 4 == 0 and w % 4 == 0: 16-byte aligned, ox + 3 < w
                qx[r] = *reinterpret_cast<const rm_i32x4 *>(mqx + i); qy[r] = *reinterpret_cast<const rm_i32x4 *>(mqy + i);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (ox + k < w) { qx[r][k] = mqx[i + k]; qy[r][k] = mqy[i + k]; }
            }
        }
    }
}

// the box of a tile: the source pixels its in-picture taps touch (a tap is (sy, sx) .. (sy + 1, sx + 1)).  x0a: the left edge on a 16-pixel
// boundary; pitch: its width in whole groups of 16; rows > 0: staged in LDS (pitch * rows <= RM_LDS), rows < 0: -rows rows that do not fit
// (gathered from global memory), rows == 0: no tap inside the picture
struct RemapBox { int x0a, y0, pitch, rows; };

// all 256 lanes: the box of the tile whose map entries the lanes hold (s_box: 64 bytes of LDS; ends behind a barrier)
__device__ __forceinline__ RemapBox remap_reduce_box(const rm_i32x4 (&qx)[2], const rm_i32x4 (&qy)[2], int w, int h, int (*s_box)[4])
{
    int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (qx[r][k] != RM_OUTSIDE) {
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
    RemapBox B;
    B.x0a = any ? (x0 & ~15) : 0; B.y0 = any ? y0 : 0;
    B.pitch = any ? ((x1 - B.x0a + 16) & ~15) : 16;
    const int rows = any ? y1 - y0 + 1 : 0;
    B.rows = (long long)B.pitch * rows <= RM_LDS ? rows : -rows;
    return B;
}

// all 256 lanes: the lane's 2 x 4 pixels of one tile of one slot.  tile: RM_LDS bytes of LDS, 16-byte aligned; s: the slot's picture [h][w][channels]
// (channels 1 or 3), d: its level 0 [h][w]; qx, qy: remap_load_q's entries at (ox, oy0); B: the tile's box.  The box is staged in LDS (BGR -> gray
// once per source pixel); one that does not fit is gathered from global memory instead.  Dword stores where w % 4 == 0
__device__ __forceinline__ void remap_tile(uint8_t *tile, const uint8_t *s, uint8_t *d, const rm_i32x4 (&qx)[2],
                                           const rm_i32x4 (&qy)[2], const RemapBox &B, int w, int h, int channels, int border, int ox, int oy0)
{
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
                    o[q] = remap_gray1(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u) | (remap_gray1(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u) << 8) |
                           (remap_gray1((w1 >> 16) & 255u, w1 >> 24, w2 & 255u) << 16) | (remap_gray1((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24) << 24);
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
                            o[q] |= (channels == 3 ? remap_gray1(t[0], t[1], t[2]) : (uint32_t)t[0]) << (8 * k);
                        }
                    }
                }
            }
            *reinterpret_cast<uint4 *>(&tile[r * pitch + c]) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }
    // a tap outside the picture is the border value; one inside lies in the staged box by construction of the box, and the mask keeps a box
    // that was read from memory from indexing past the tile whatever it holds
    auto tap = [&](int y, int x) -> int {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return border;
        if (staged) return (int)tile[((y - y0) * pitch + (x - x0a)) & (RM_LDS - 1)];
        const uint8_t *t = s + ((size_t)y * w + x) * (size_t)channels;
        return channels == 3 ? (int)remap_gray1(t[0], t[1], t[2]) : (int)t[0];
    };
    const bool w4 = (w & 3) == 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 16 * r;
        if (oy >= h || ox >= w) continue;
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = (uint32_t)border;
            if (qx[r][k] != RM_OUTSIDE) {
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
