// Projection-guided descriptor search: the primitive under ORB-SLAM2's ORBmatcher::SearchBySim3, SearchByProjection(pKF, Scw, points, ...)
// and Fuse(pKF, Scw, points, ...) -- nothing in the reference, whose LoopClosing is empty.  A problem is one target
// keyframe (keypoints: level-0 pixel, level, descriptor, optional taken flag) and one point set (world position, descriptor, scale-invariance
// distance, optional normal and skip flag) with a similarity S, world -> target camera.
//
//   k_proj_search   lane = point, block = 256 points of one problem.  The lane projects its point (skip flag, z > 0, image bounds, distance
//                   range, viewing angle, predicted level by comparisons with powers of two), then the problem's keypoints stream through LDS
//                   in tiles of 256 (k_bow_match's shape): level, taken flag and window form the mask, the 256-bit Hamming distance is
//                   evaluated only where it holds.  The lane keeps its YGZ_PROJ_TOPK best candidates as sorted keys (distance << 20 | index)
//                   in registers (a min / max ladder with constant indices: no scratch) and counts every candidate within th_dist.
//
// The claim (claim == 1: points in index order, each takes the first entry of its list that no earlier point took) is a serial chain over
// lists of one or two entries: the entry point resolves it on the host from the lists it copied back, inside the same call.
// One upload from page-locked memory, one launch, one copy back, one wait.  The arithmetic is that of tests/proj_ref.c, bit for bit.
#include "ygz_internal.h"
#include "se3_dev.h"
#include <string.h>
#include <math.h>

namespace {

#define PROJ_LANES      256
#define PROJ_TILE       256
#define PROJ_IDX_BITS   20             // key = distance << 20 | keypoint index
#define PROJ_TAKEN      0x40000000     // the level a taken keypoint is given in LDS: compatible with no predicted level

struct ProjIn { double K4[4]; double th; int32_t th_dist, w, h, L; };

struct ProjProbDev {
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const uint8_t *kp_taken;
    const double *pw; const uint32_t *pt_desc; const double *pt_dmax; const double *pt_normal; const uint8_t *pt_skip;
    int32_t n_kp, n_pt, pt_off, pad_;
    double S[8];
};

// steps 1-6 of tests/proj_ref.c's pr_project: the predicted level, or -1 for a culled point
__device__ __forceinline__ int proj_point(const ProjProbDev &P, const ProjIn &in, int i, double *u_out, double *v_out)
{
    if (P.pt_skip && P.pt_skip[i]) return -1;
    double R[9];
    quat_to_R_d(P.S, R);
    const double *X = P.pw + 3 * (size_t)i;
    const double X0 = X[0], X1 = X[1], X2 = X[2], s = P.S[7];
    const double x = s * (R[0] * X0 + R[1] * X1 + R[2] * X2) + P.S[4];
    const double y = s * (R[3] * X0 + R[4] * X1 + R[5] * X2) + P.S[5];
    const double z = s * (R[6] * X0 + R[7] * X1 + R[8] * X2) + P.S[6];
    if (!(z > 0)) return -1;
    const double iz = 1 / z;
    const double u = in.K4[0] * (x * iz) + in.K4[2], v = in.K4[1] * (y * iz) + in.K4[3];
    if (!(u >= 0 && u < (double)in.w && v >= 0 && v < (double)in.h)) return -1;
    const double d = sqrt(x * x + y * y + z * z);
    const double dmax = P.pt_dmax[i], dmin = dmax / (double)(1 << (in.L - 1));
    if (d < 0.8 * dmin || d > 1.2 * dmax) return -1;
    if (P.pt_normal) {
        const double *n = P.pt_normal + 3 * (size_t)i;
        const double n0 = n[0], n1 = n[1], n2 = n[2];
        const double nx = R[0] * n0 + R[1] * n1 + R[2] * n2;
        const double ny = R[3] * n0 + R[4] * n1 + R[5] * n2;
        const double nz = R[6] * n0 + R[7] * n1 + R[8] * n2;
        if (x * nx + y * ny + z * nz < 0.5 * d) return -1;
    }
    const double ratio = dmax / d;
    int pred = in.L - 1;
    for (int n = in.L - 2; n >= 0; --n)
        if (ratio <= (double)(1 << n)) pred = n;
    *u_out = u; *v_out = v;
    return pred;
}

__global__ __launch_bounds__(PROJ_LANES) void k_proj_search(const ProjIn *__restrict__ in_, const ProjProbDev *__restrict__ probs,
                                                            uint32_t *__restrict__ keys, int32_t *__restrict__ n_cand,
                                                            int32_t *__restrict__ pred_level)
{
    __shared__ uint32_t s_d[PROJ_TILE][9];        // descriptor + level (pitch 9: conflict-free broadcast reads)
    __shared__ double s_p[PROJ_TILE][2];
    const ProjProbDev &P = probs[blockIdx.y];
    if ((int)(blockIdx.x * PROJ_LANES) >= P.n_pt) return;
    const ProjIn in = *in_;
    const int i = blockIdx.x * PROJ_LANES + threadIdx.x;
    const bool live = i < P.n_pt;
    double u = 0, v = 0;
    const int pred = live ? proj_point(P, in, i, &u, &v) : -1;
    uint32_t key[YGZ_PROJ_TOPK];
#pragma unroll
    for (int m = 0; m < YGZ_PROJ_TOPK; ++m) key[m] = 0xFFFFFFFFu;
    int n = 0;
    if (__syncthreads_or(pred >= 0)) {
        uint32_t d[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (pred >= 0) {
            const uint4 a = *reinterpret_cast<const uint4 *>(P.pt_desc + 8 * (size_t)i), b = *reinterpret_cast<const uint4 *>(P.pt_desc + 8 * (size_t)i + 4);
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
        }
        const double rad = in.th * (double)(1 << (pred < 0 ? 0 : pred));
        const int n_kp = P.n_kp;
        for (int j0 = 0; j0 < n_kp; j0 += PROJ_TILE) {
            const int j = j0 + (int)threadIdx.x;
            __syncthreads();
            if (j < n_kp) {
                const uint4 a = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j), b = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j + 4);
                uint32_t *r = s_d[threadIdx.x];
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
                r[8] = (P.kp_taken && P.kp_taken[j]) ? (uint32_t)PROJ_TAKEN : (uint32_t)P.kp_level[j];
                s_p[threadIdx.x][0] = P.kp_px[2 * (size_t)j]; s_p[threadIdx.x][1] = P.kp_px[2 * (size_t)j + 1];
            }
            __syncthreads();
            if (pred < 0) continue;
            const int cnt = min(PROJ_TILE, n_kp - j0);
            for (int t = 0; t < cnt; ++t) {
                const uint32_t *r = s_d[t];
                const int lv = (int)r[8];
                if (lv < pred - 1 || lv > pred) continue;
                const double dx = s_p[t][0] - u, dy = s_p[t][1] - v;
                if (!(dx < rad && dx > -rad && dy < rad && dy > -rad)) continue;
                const int dist = __popc(d[0] ^ r[0]) + __popc(d[1] ^ r[1]) + __popc(d[2] ^ r[2]) + __popc(d[3] ^ r[3]) +
                                 __popc(d[4] ^ r[4]) + __popc(d[5] ^ r[5]) + __popc(d[6] ^ r[6]) + __popc(d[7] ^ r[7]);
                if (dist > in.th_dist) continue;
                ++n;
                uint32_t k = ((uint32_t)dist << PROJ_IDX_BITS) | (uint32_t)(j0 + t);
#pragma unroll
                for (int m = 0; m < YGZ_PROJ_TOPK; ++m) { const uint32_t lo = min(key[m], k); k = max(key[m], k); key[m] = lo; }
            }
        }
    }
    if (!live) return;
    const size_t g = (size_t)P.pt_off + (size_t)i;
    uint4 *o = reinterpret_cast<uint4 *>(keys + YGZ_PROJ_TOPK * g);
    o[0] = make_uint4(key[0], key[1], key[2], key[3]);
    o[1] = make_uint4(key[4], key[5], key[6], key[7]);
    n_cand[g] = n;
    pred_level[g] = pred;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct Out { const uint32_t *keys; const int32_t *n_cand, *pred; };

// validation (before anything touches the device), one upload, the launch, one copy back, one wait; `out` points into the page-locked copy
int run(ygz_hip_ctx *ctx, int P, const ygz_proj_problem *pb, const double *K4, const ygz_proj_params *params, ygz_proj_params *used, Out *out)
{
    if (!ctx || !pb || !K4 || P < 1) return YGZ_E_INVALID;
    if (P > YGZ_PROJ_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    ygz_proj_params p;
    if (params) p = *params; else ygz_hip_default_proj_params(&p);
    if (!(p.th > 0) || !std::isfinite(p.th) || p.th_dist < 0 || p.th_dist > 256) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    bool big = false;
    size_t N = 0;
    for (int q = 0; q < P; ++q) {
        const ygz_proj_problem &b = pb[q];
        if (!b.kp_px || !b.kp_level || !b.kp_desc || !b.pw || !b.pt_desc || !b.pt_dmax || b.n_kp < 1 || b.n_pt < 1) return YGZ_E_INVALID;
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(b.S[k])) return YGZ_E_INVALID;
        if (!(b.S[7] > 0)) return YGZ_E_INVALID;
        big = big || b.n_kp > ctx->cells || b.n_kp > (1 << PROJ_IDX_BITS);
        N += (size_t)b.n_pt;
    }
    if (big || N > YGZ_PROJ_MAX_POINTS) return YGZ_E_CAPACITY;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }

    // the layout: [in | problems | every problem's arrays) goes up, [keys | n_cand | pred) comes back
    YgzBlobLayout B;
    const size_t o_in = B.add(sizeof(ProjIn)), o_pb = B.add_n<ProjProbDev>((size_t)P);
    struct Offs { size_t kp_px, kp_level, kp_desc, kp_taken, pw, pt_desc, pt_dmax, pt_normal, pt_skip; };
    Offs of[YGZ_PROJ_MAX_PROBLEMS];
    int max_pt = 0;
    for (int q = 0; q < P; ++q) {
        const ygz_proj_problem &b = pb[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)b.n_pt;
        of[q].kp_px = B.add_n<double>(nk * 2);
        of[q].kp_level = B.add_n<int32_t>(nk);
        of[q].kp_desc = B.add_n<uint32_t>(nk * 8);
        of[q].kp_taken = B.add(b.kp_taken ? nk : 0);         // the optional arrays take no room when absent
        of[q].pw = B.add_n<double>(np * 3);
        of[q].pt_desc = B.add_n<uint32_t>(np * 8);
        of[q].pt_dmax = B.add_n<double>(np);
        of[q].pt_normal = B.add_n<double>(b.pt_normal ? np * 3 : 0);
        of[q].pt_skip = B.add(b.pt_skip ? np : 0);
        if (b.n_pt > max_pt) max_pt = b.n_pt;
    }
    const size_t in_end = B.end;
    const size_t o_keys = B.add_n<uint32_t>(N * YGZ_PROJ_TOPK), o_nc = B.add_n<int32_t>(N), o_pred = B.add_n<int32_t>(N), total = B.end;
    YgzBlob blob;                                           // [0, in_end) goes up, [keys, total) comes back
    int rc = ygz_blob_open(ctx, SCR_PROJ, total, total, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    ProjIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.th = p.th; in.th_dist = p.th_dist; in.w = ctx->prm.image_width; in.h = ctx->prm.image_height; in.L = L;
    memcpy(up + o_in, &in, sizeof in);
    size_t off = 0;
    for (int q = 0; q < P; ++q) {
        const ygz_proj_problem &b = pb[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)b.n_pt;
        memcpy(up + of[q].kp_px, b.kp_px, nk * 16);
        memcpy(up + of[q].kp_level, b.kp_level, nk * 4);
        memcpy(up + of[q].kp_desc, b.kp_desc, nk * 32);
        if (b.kp_taken) memcpy(up + of[q].kp_taken, b.kp_taken, nk);
        memcpy(up + of[q].pw, b.pw, np * 24);
        memcpy(up + of[q].pt_desc, b.pt_desc, np * 32);
        memcpy(up + of[q].pt_dmax, b.pt_dmax, np * 8);
        if (b.pt_normal) memcpy(up + of[q].pt_normal, b.pt_normal, np * 24);
        if (b.pt_skip) memcpy(up + of[q].pt_skip, b.pt_skip, np);
        ProjProbDev D;
        memset(&D, 0, sizeof D);
        D.kp_px = ygz_at<const double>(dev, of[q].kp_px); D.kp_level = ygz_at<const int32_t>(dev, of[q].kp_level);
        D.kp_desc = ygz_at<const uint32_t>(dev, of[q].kp_desc); D.kp_taken = b.kp_taken ? dev + of[q].kp_taken : nullptr;
        D.pw = ygz_at<const double>(dev, of[q].pw); D.pt_desc = ygz_at<const uint32_t>(dev, of[q].pt_desc);
        D.pt_dmax = ygz_at<const double>(dev, of[q].pt_dmax); D.pt_normal = b.pt_normal ? ygz_at<const double>(dev, of[q].pt_normal) : nullptr;
        D.pt_skip = b.pt_skip ? dev + of[q].pt_skip : nullptr;
        D.n_kp = b.n_kp; D.n_pt = b.n_pt; D.pt_off = (int32_t)off;
        for (int k = 0; k < 8; ++k) D.S[k] = b.S[k];
        memcpy(up + o_pb + (size_t)q * sizeof(ProjProbDev), &D, sizeof D);
        off += np;
    }
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;
    YGZ_LAUNCH(ctx, KID_COUNT, k_proj_search, dim3(ygz_div_up(max_pt, PROJ_LANES), P), dim3(PROJ_LANES), ygz_at<const ProjIn>(dev, o_in),
               ygz_at<const ProjProbDev>(dev, o_pb), ygz_at<uint32_t>(dev, o_keys), ygz_at<int32_t>(dev, o_nc), ygz_at<int32_t>(dev, o_pred));
    if ((rc = ygz_blob_fetch(ctx, blob, o_keys, total)) != YGZ_OK) return rc;
    out->keys = ygz_at<const uint32_t>(up, o_keys);
    out->n_cand = ygz_at<const int32_t>(up, o_nc);
    out->pred = ygz_at<const int32_t>(up, o_pred);
    *used = p;
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_proj_params(ygz_proj_params *p)
{
    if (!p) return;
    p->th = 10.0; p->th_dist = 50; p->claim = 1;
}

int ygz_hip_search_by_projection(ygz_hip_ctx *ctx, int n_problems, const ygz_proj_problem *problems, const double K4[4],
                                 const ygz_proj_params *params, int32_t *match, int32_t *dist, int32_t *pred_level, int32_t *counts)
{
    Out o;
    ygz_proj_params p;
    const int rc = run(ctx, n_problems, problems, K4, params, &p, &o);
    if (rc != YGZ_OK) return rc;
    // the claim, on the lists that came back: a point's entries are sorted by (distance, index), so the best unclaimed candidate is the first
    // unclaimed entry
    std::vector<uint8_t> taken;
    size_t off = 0;
    for (int q = 0; q < n_problems; ++q) {
        const int np = problems[q].n_pt;
        if (p.claim) taken.assign((size_t)problems[q].n_kp, 0);
        int nm = 0, nov = 0;
        for (int i = 0; i < np; ++i) {
            const size_t g = off + (size_t)i;
            const uint32_t *key = o.keys + YGZ_PROJ_TOPK * g;
            const int n = o.n_cand[g] < YGZ_PROJ_TOPK ? o.n_cand[g] : YGZ_PROJ_TOPK;
            if (o.n_cand[g] > YGZ_PROJ_TOPK) ++nov;
            int m = -1, dd = -1;
            for (int k = 0; k < n; ++k) {
                const int j = (int)(key[k] & ((1u << PROJ_IDX_BITS) - 1));
                if (p.claim && taken[j]) continue;
                m = j; dd = (int)(key[k] >> PROJ_IDX_BITS);
                break;
            }
            if (m >= 0) { ++nm; if (p.claim) taken[m] = 1; }
            if (match) match[g] = m;
            if (dist) dist[g] = dd;
        }
        if (pred_level) memcpy(pred_level + off, o.pred + off, (size_t)np * 4);
        if (counts) { counts[2 * q] = nm; counts[2 * q + 1] = nov; }
        off += (size_t)np;
    }
    return YGZ_OK;
}

int ygz_hip_projection_candidates(ygz_hip_ctx *ctx, const ygz_proj_problem *problem, const double K4[4], const ygz_proj_params *params,
                                  int32_t *cand_idx, int32_t *cand_dist, int32_t *n_cand, int32_t *pred_level)
{
    Out o;
    ygz_proj_params p;
    const int rc = run(ctx, 1, problem, K4, params, &p, &o);
    if (rc != YGZ_OK) return rc;
    const int np = problem->n_pt;
    for (int i = 0; i < np; ++i) {
        const int n = o.n_cand[i] < YGZ_PROJ_TOPK ? o.n_cand[i] : YGZ_PROJ_TOPK;
        for (int k = 0; k < YGZ_PROJ_TOPK; ++k) {
            const uint32_t key = o.keys[(size_t)YGZ_PROJ_TOPK * i + k];
            if (cand_idx) cand_idx[(size_t)YGZ_PROJ_TOPK * i + k] = k < n ? (int32_t)(key & ((1u << PROJ_IDX_BITS) - 1)) : -1;
            if (cand_dist) cand_dist[(size_t)YGZ_PROJ_TOPK * i + k] = k < n ? (int32_t)(key >> PROJ_IDX_BITS) : -1;
        }
    }
    if (n_cand) memcpy(n_cand, o.n_cand, (size_t)np * 4);
    if (pred_level) memcpy(pred_level, o.pred, (size_t)np * 4);
    return YGZ_OK;
}

}  // extern "C"
