// LF -- local-map fusion search: the search of ORB-SLAM2's ORBmatcher::Fuse(pKF, vpMapPoints, th) as LocalMapping::SearchInNeighbors calls it.
// Nothing in the reference.  ygz_hip_search_by_projection (proj.hip) cannot serve: it has no per-candidate pixel gate, and it uploads the point
// set once per problem, while here up to 64 target keyframes look at the SAME points.  The frozen spec is tests/lfuse_ref.c (DESIGN.md section
// 25): FP64, uncontracted + - * / and sqrt in one stated order; every output is bit-identical to it.
//   k_lfuse_search  k_proj_search's shape: lane = one (problem, point), block = 256 points of one problem (blockIdx.y), all problems of the call
//                   in one launch; the point sets are in the block once and every problem names its set.  The lane projects its point (steps
//                   1-6b: skip flag, z > 0, image bounds, distance range, viewing angle, predicted level, the right column ur = u - bf / z),
//                   then the problem's keypoints stream through LDS in tiles of 256, 64 bytes each (pixel, right column, level; descriptor).
//                   Level and window are tested first (eight tile entries at a time without a branch, so that their LDS reads are in flight
//                   together: with less than one wavefront per SIMD nothing else hides that latency), then the chi2 gate (with the right
//                   column on a stereo keypoint), and the 256-bit Hamming distance is evaluated only where all three hold.  The best survivor
//                   is ONE key (distance << 20 | index) in a register.  A block whose points are all culled skips the sweep.
// No atomic, no wait for another workgroup, no scratch, no environment switch.  One packed upload, one launch, one copy back, one wait.
#include "ygz_internal.h"
#include "se3_dev.h"
#include <math.h>
#include <string.h>
#include "pose_block.h"                 // ygz_all_finite
#pragma clang fp contract(off)

#define LF_LANES     256
#define LF_TILE      256
#define LF_GROUP     8                  // tile entries whose level and window are tested together
#define LF_IDX_BITS  20                 // key = distance << 20 | keypoint index
#define LF_TAKEN     0x40000000         // the level a taken keypoint is given in LDS: compatible with no predicted level
#define LF_NO_KEY    0xFFFFFFFFu

struct LfIn { double K4[4]; double th, bf, chi2_mono, chi2_stereo; int32_t th_dist, w, h, L; };

struct LfSetDev { const double *pw; const uint32_t *pt_desc; const double *pt_dmax; const double *pt_normal; int32_t n_pt, pad_; };

struct LfProbDev {
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const double *kp_ur; const uint8_t *kp_taken; const uint8_t *pt_skip;
    int32_t n_kp, set, pt_off, pad_;
    double T[7];
};

struct LfKp { double kx, ky, ur; int32_t level, pad_; };     // 32 bytes; the descriptor is another 32

namespace {

// steps 1-6b of tests/lfuse_ref.c (pr_project of tests/proj_ref.c with s = 1: a factor 1.0 changes no bit): the reason, and for reason 0 the
// pixel, the right column and the predicted level
__device__ __forceinline__ int lf_point(const LfSetDev &S, const LfProbDev &P, const LfIn &in, int i, double *u_out, double *v_out, double *ur_out,
                                        int *pred_out)
{
    *pred_out = -1;
    if (P.pt_skip && P.pt_skip[i]) return 1;
    double R[9];
    quat_to_R_d(P.T, R);
    const double *X = S.pw + 3 * (size_t)i;
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double x = (R[0] * X0 + R[1] * X1 + R[2] * X2) + P.T[4];
    const double y = (R[3] * X0 + R[4] * X1 + R[5] * X2) + P.T[5];
    const double z = (R[6] * X0 + R[7] * X1 + R[8] * X2) + P.T[6];
    if (!(z > 0)) return 2;
    const double iz = 1 / z;
    const double u = in.K4[0] * (x * iz) + in.K4[2], v = in.K4[1] * (y * iz) + in.K4[3];
    if (!(u >= 0 && u < (double)in.w && v >= 0 && v < (double)in.h)) return 3;
    const double d = sqrt(x * x + y * y + z * z);
    const double dmax = S.pt_dmax[i], dmin = dmax / (double)(1 << (in.L - 1));
    if (d < 0.8 * dmin || d > 1.2 * dmax) return 4;
    if (S.pt_normal) {
        const double *n = S.pt_normal + 3 * (size_t)i;
        const double n0 = n[0], n1 = n[1], n2 = n[2];
        const double nx = R[0] * n0 + R[1] * n1 + R[2] * n2;
        const double ny = R[3] * n0 + R[4] * n1 + R[5] * n2;
        const double nz = R[6] * n0 + R[7] * n1 + R[8] * n2;
        if (x * nx + y * ny + z * nz < 0.5 * d) return 5;
    }
    const double ratio = dmax / d;
    int pred = in.L - 1;
    for (int n = in.L - 2; n >= 0; --n)
        if (ratio <= (double)(1 << n)) pred = n;
    *u_out = u; *v_out = v; *ur_out = u - in.bf * iz; *pred_out = pred;
    return 0;
}

}  // namespace

__global__ __launch_bounds__(LF_LANES) void k_lfuse_search(const LfIn *__restrict__ in_, const LfSetDev *__restrict__ sets,
                                                           const LfProbDev *__restrict__ probs, int32_t *__restrict__ match,
                                                           int32_t *__restrict__ dist_out, int32_t *__restrict__ pred_level,
                                                           int32_t *__restrict__ reason, int32_t *__restrict__ n_gated)
{
    __shared__ LfKp s_k[LF_TILE];
    __shared__ uint4 s_d[LF_TILE][2];
    const LfProbDev &P = probs[blockIdx.y];
    const LfSetDev &S = sets[P.set];
    const int n_pt = S.n_pt;
    if ((int)(blockIdx.x * LF_LANES) >= n_pt) return;              // the same in every lane of the block
    const LfIn in = *in_;
    const int i = blockIdx.x * LF_LANES + threadIdx.x;
    const bool live = i < n_pt;
    double u = 0, v = 0, ur = 0;
    int pred = -1;
    const int why = live ? lf_point(S, P, in, i, &u, &v, &ur, &pred) : 1;
    uint32_t best = LF_NO_KEY;
    int ng = 0;
    if (__syncthreads_or(pred >= 0)) {
        uint32_t d[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (pred >= 0) {
            const uint4 a = *reinterpret_cast<const uint4 *>(S.pt_desc + 8 * (size_t)i), b = *reinterpret_cast<const uint4 *>(S.pt_desc + 8 * (size_t)i + 4);
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
        }
        const double rad = in.th * (double)(1 << (pred < 0 ? 0 : pred));
        const int n_kp = P.n_kp;
        for (int j0 = 0; j0 < n_kp; j0 += LF_TILE) {
            const int j = j0 + (int)threadIdx.x;
            __syncthreads();
            if (j >= n_kp) s_k[threadIdx.x].level = (int32_t)LF_TAKEN;     // past the end: in no window (the sweep goes in groups of LF_GROUP)
            else {
                LfKp k;
                k.kx = P.kp_px[2 * (size_t)j]; k.ky = P.kp_px[2 * (size_t)j + 1];
                k.ur = P.kp_ur ? P.kp_ur[j] : -1.0;
                k.level = (P.kp_taken && P.kp_taken[j]) ? (int32_t)LF_TAKEN : P.kp_level[j];
                k.pad_ = 0;
                s_k[threadIdx.x] = k;
                s_d[threadIdx.x][0] = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j);
                s_d[threadIdx.x][1] = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j + 4);
            }
            __syncthreads();
            if (pred < 0) continue;
            const int cnt = min(LF_TILE, n_kp - j0);
            // level and window of LF_GROUP entries at a time, without a branch: their LDS reads (one address for all lanes: broadcasts) are in
            // flight together; the gate and the Hamming distance only for the entries whose bit is set, in index order
            for (int t0 = 0; t0 < cnt; t0 += LF_GROUP) {
                uint32_t in_window = 0;
                int glv[LF_GROUP];
                double gx[LF_GROUP], gy[LF_GROUP];
#pragma unroll
                for (int g = 0; g < LF_GROUP; ++g) { glv[g] = s_k[t0 + g].level; gx[g] = s_k[t0 + g].kx; gy[g] = s_k[t0 + g].ky; }
#pragma unroll
                for (int g = 0; g < LF_GROUP; ++g) {
                    const int lv = glv[g];
                    const double dx = gx[g] - u, dy = gy[g] - v;
                    const uint32_t ok = (uint32_t)(lv >= pred - 1) & (uint32_t)(lv <= pred) & (uint32_t)(dx < rad) & (uint32_t)(dx > -rad) &
                                        (uint32_t)(dy < rad) & (uint32_t)(dy > -rad);
                    in_window |= ok << g;
                }
                while (in_window) {
                    const int t = t0 + __ffs((int)in_window) - 1;
                    in_window &= in_window - 1;
                    const int lv = s_k[t].level;
                    const double kx = s_k[t].kx, ky = s_k[t].ky;
                    const double ex = u - kx, ey = v - ky, s2 = (double)(1 << (2 * lv));
                    double e2 = ex * ex + ey * ey;
                    const double kur = s_k[t].ur;
                    bool out;
                    if (kur >= 0) {
                        const double er = ur - kur;
                        e2 = e2 + er * er;
                        out = e2 > in.chi2_stereo * s2;
                    } else out = e2 > in.chi2_mono * s2;
                    if (out) { ++ng; continue; }
                    const uint4 a = s_d[t][0], b = s_d[t][1];
                    const int dist = __popc(d[0] ^ a.x) + __popc(d[1] ^ a.y) + __popc(d[2] ^ a.z) + __popc(d[3] ^ a.w) +
                                     __popc(d[4] ^ b.x) + __popc(d[5] ^ b.y) + __popc(d[6] ^ b.z) + __popc(d[7] ^ b.w);
                    best = min(best, ((uint32_t)dist << LF_IDX_BITS) | (uint32_t)(j0 + t));
                }
            }
        }
    }
    if (!live) return;
    const size_t g = (size_t)P.pt_off + (size_t)i;
    const int bd = (int)(best >> LF_IDX_BITS);
    const bool hit = best != LF_NO_KEY && bd <= in.th_dist;
    match[g] = hit ? (int32_t)(best & ((1u << LF_IDX_BITS) - 1)) : -1;
    dist_out[g] = hit ? bd : -1;
    pred_level[g] = pred;
    reason[g] = why;
    n_gated[g] = ng;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

void ygz_hip_default_lfuse_params(ygz_lfuse_params *p)
{
    if (!p) return;
    p->th = 3.0; p->baseline = 0.1; p->chi2_mono = 5.99; p->chi2_stereo = 7.8; p->th_dist = 50; p->pad = 0;
}

int ygz_hip_local_fuse_search(ygz_hip_ctx *ctx, int n_sets, const ygz_lfuse_points *sets, int n_problems, const ygz_lfuse_problem *problems,
                              const double K4[4], const ygz_lfuse_params *params, int32_t *match, int32_t *dist, int32_t *pred_level,
                              int32_t *reason, int32_t *n_gated, int32_t *counts)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!sets || !problems || !K4 || n_sets < 1 || n_problems < 1) return YGZ_E_INVALID;
    if (n_sets > YGZ_LFUSE_MAX_SETS || n_problems > YGZ_LFUSE_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    for (int s = 0; s < n_sets; ++s) {
        if (sets[s].n_pt < 0) return YGZ_E_INVALID;
        if (sets[s].n_pt > 0 && (!sets[s].pw || !sets[s].pt_desc || !sets[s].pt_dmax)) return YGZ_E_INVALID;
    }
    size_t N = 0;
    bool big = false;
    int max_pt = 0;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_lfuse_problem &b = problems[q];
        if (b.set < 0 || b.set >= n_sets || b.n_kp < 1 || !b.kp_px || !b.kp_level || !b.kp_desc) return YGZ_E_INVALID;
        big = big || b.n_kp > (1 << LF_IDX_BITS);
        N += (size_t)sets[b.set].n_pt;
        if (sets[b.set].n_pt > max_pt) max_pt = sets[b.set].n_pt;
    }
    if (big || N > YGZ_LFUSE_MAX_PAIRS) return YGZ_E_CAPACITY;
    ygz_lfuse_params p;
    if (params) p = *params; else ygz_hip_default_lfuse_params(&p);
    if (!isfinite(p.th) || !isfinite(p.baseline) || !isfinite(p.chi2_mono) || !isfinite(p.chi2_stereo)) return YGZ_E_INVALID;
    if (!(p.th > 0) || !(p.baseline > 0) || !(p.chi2_mono > 0) || !(p.chi2_stereo > 0) || p.th_dist < 0 || p.th_dist > 256) return YGZ_E_INVALID;
    if (!ygz_all_finite(K4, 4) || !(K4[0] > 0) || !(K4[1] > 0)) return YGZ_E_INVALID;
    for (int s = 0; s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        if (!n) continue;
        if (!ygz_all_finite(sets[s].pw, 3 * n) || !ygz_all_finite(sets[s].pt_dmax, n)) return YGZ_E_INVALID;
    }
    for (int q = 0; q < n_problems; ++q) {
        if (!ygz_all_finite(problems[q].T, 7)) return YGZ_E_INVALID;
        if (problems[q].kp_ur && !ygz_all_finite(problems[q].kp_ur, (size_t)problems[q].n_kp)) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    for (int q = 0; q < n_problems; ++q) {
        if (problems[q].n_kp > ctx->cells) return YGZ_E_CAPACITY;
        for (int j = 0; j < problems[q].n_kp; ++j)
            if (problems[q].kp_level[j] < 0 || problems[q].kp_level[j] >= L) return YGZ_E_INVALID;
    }
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (counts) memset(counts, 0, (size_t)n_problems * 2 * sizeof(int32_t));
    if (N == 0) return YGZ_OK;                                      // nothing to search: no launch

    // up: [in | sets | problems | every set's arrays | every problem's arrays), back: [match | dist | pred | reason | n_gated)
    const size_t Q = (size_t)n_problems;
    YgzBlobLayout B;
    const size_t o_in = B.add(sizeof(LfIn)), o_sets = B.add_n<LfSetDev>((size_t)n_sets), o_pb = B.add_n<LfProbDev>(Q);
    struct SetOffs { size_t pw, desc, dmax, normal; };
    struct ProbOffs { size_t px, level, desc, ur, taken, skip; };
    SetOffs so[YGZ_LFUSE_MAX_SETS];
    ProbOffs po[YGZ_LFUSE_MAX_PROBLEMS];
    for (int s = 0; s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        so[s].pw = B.add_n<double>(n * 3);
        so[s].desc = B.add_n<uint4>(n * 2);                        // 16-byte aligned: read as two uint4
        so[s].dmax = B.add_n<double>(n);
        so[s].normal = B.add_n<double>(sets[s].pt_normal ? n * 3 : 0);
    }
    for (int q = 0; q < n_problems; ++q) {
        const ygz_lfuse_problem &b = problems[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)sets[b.set].n_pt;
        po[q].px = B.add_n<double>(nk * 2);
        po[q].level = B.add_n<int32_t>(nk);
        po[q].desc = B.add_n<uint4>(nk * 2);
        po[q].ur = B.add_n<double>(b.kp_ur ? nk : 0);              // the optional arrays take no room when absent
        po[q].taken = B.add(b.kp_taken ? nk : 0);
        po[q].skip = B.add(b.pt_skip ? np : 0);
    }
    const size_t in_end = B.end;
    const size_t o_match = B.add_n<int32_t>(N), o_dist = B.add_n<int32_t>(N), o_pred = B.add_n<int32_t>(N), o_why = B.add_n<int32_t>(N);
    const size_t o_ng = B.add_n<int32_t>(N), total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_LFUSE, total, total, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    LfIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.th = p.th; in.bf = K4[0] * p.baseline; in.chi2_mono = p.chi2_mono; in.chi2_stereo = p.chi2_stereo;
    in.th_dist = p.th_dist; in.w = ctx->prm.image_width; in.h = ctx->prm.image_height; in.L = L;
    memcpy(up + o_in, &in, sizeof in);
    for (int s = 0; s < n_sets; ++s) {
        const ygz_lfuse_points &b = sets[s];
        const size_t n = (size_t)b.n_pt;
        LfSetDev D;
        memset(&D, 0, sizeof D);
        if (n) {
            memcpy(up + so[s].pw, b.pw, n * 24); memcpy(up + so[s].desc, b.pt_desc, n * 32); memcpy(up + so[s].dmax, b.pt_dmax, n * 8);
            if (b.pt_normal) memcpy(up + so[s].normal, b.pt_normal, n * 24);
        }
        D.pw = ygz_at<const double>(dev, so[s].pw); D.pt_desc = ygz_at<const uint32_t>(dev, so[s].desc);
        D.pt_dmax = ygz_at<const double>(dev, so[s].dmax); D.pt_normal = b.pt_normal ? ygz_at<const double>(dev, so[s].normal) : nullptr;
        D.n_pt = b.n_pt;
        memcpy(up + o_sets + (size_t)s * sizeof(LfSetDev), &D, sizeof D);
    }
    std::vector<size_t> offs(Q + 1, 0);
    for (int q = 0; q < n_problems; ++q) {
        const ygz_lfuse_problem &b = problems[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)sets[b.set].n_pt;
        memcpy(up + po[q].px, b.kp_px, nk * 16); memcpy(up + po[q].level, b.kp_level, nk * 4); memcpy(up + po[q].desc, b.kp_desc, nk * 32);
        if (b.kp_ur) memcpy(up + po[q].ur, b.kp_ur, nk * 8);
        if (b.kp_taken) memcpy(up + po[q].taken, b.kp_taken, nk);
        if (b.pt_skip && np) memcpy(up + po[q].skip, b.pt_skip, np);
        LfProbDev D;
        memset(&D, 0, sizeof D);
        D.kp_px = ygz_at<const double>(dev, po[q].px); D.kp_level = ygz_at<const int32_t>(dev, po[q].level);
        D.kp_desc = ygz_at<const uint32_t>(dev, po[q].desc); D.kp_ur = b.kp_ur ? ygz_at<const double>(dev, po[q].ur) : nullptr;
        D.kp_taken = b.kp_taken ? dev + po[q].taken : nullptr; D.pt_skip = b.pt_skip ? dev + po[q].skip : nullptr;
        D.n_kp = b.n_kp; D.set = b.set; D.pt_off = (int32_t)offs[q];
        for (int k = 0; k < 7; ++k) D.T[k] = b.T[k];
        memcpy(up + o_pb + (size_t)q * sizeof(LfProbDev), &D, sizeof D);
        offs[q + 1] = offs[q] + np;
    }
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;
    YGZ_LAUNCH(ctx, KID_LFUSE_SEARCH, k_lfuse_search, dim3((unsigned)ygz_div_up(max_pt, LF_LANES), (unsigned)n_problems), dim3(LF_LANES),
               ygz_at<const LfIn>(dev, o_in), ygz_at<const LfSetDev>(dev, o_sets), ygz_at<const LfProbDev>(dev, o_pb), ygz_at<int32_t>(dev, o_match),
               ygz_at<int32_t>(dev, o_dist), ygz_at<int32_t>(dev, o_pred), ygz_at<int32_t>(dev, o_why), ygz_at<int32_t>(dev, o_ng));
    if ((rc = ygz_blob_fetch(ctx, blob, o_match, total)) != YGZ_OK) return rc;
    const int32_t *m = ygz_at<const int32_t>(up, o_match), *why = ygz_at<const int32_t>(up, o_why);
    if (match) memcpy(match, m, N * 4);
    if (dist) memcpy(dist, up + o_dist, N * 4);
    if (pred_level) memcpy(pred_level, up + o_pred, N * 4);
    if (reason) memcpy(reason, why, N * 4);
    if (n_gated) memcpy(n_gated, up + o_ng, N * 4);
    if (counts)
        for (int q = 0; q < n_problems; ++q)
            for (size_t g = offs[q]; g < offs[q + 1]; ++g) {
                if (m[g] >= 0) ++counts[2 * q];
                if (why[g] == 0) ++counts[2 * q + 1];
            }
    return YGZ_OK;
}

}  // extern "C"
