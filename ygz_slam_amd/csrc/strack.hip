// ST -- stereo tracking search: ORB-SLAM2's two tracking searches on one kernel, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th,
// bMono) (mode 0, FRAME) and SearchByProjection(F, vpMapPoints, th) (mode 1, LOCAL).  Nothing in the reference, whose tracker is monocular and
// descriptor-free.  ygz_hip_search_by_projection (proj.hip) has no right-column test and no frame-to-frame form; ygz_hip_local_fuse_search
// (lfuse.hip) has no list, so no claim, no second best and no ratio test.  The frozen spec is tests/strack_ref.c: FP64,
// uncontracted + - * / and sqrt in one stated order; every output is bit-identical to it.
//   k_strack_search  k_lfuse_search's shape: lane = one (problem, point), block = 256 points of one problem (blockIdx.y), all problems of the
//                    call in one launch; the point sets are in the block once and every problem names its set.  The lane projects its point
//                    (skip flag, z > 0, image bounds, the right column ur = u - bf / z; FRAME: the feature's level, the level range of the
//                    motion direction; LOCAL: distance range, viewing angle, predicted level, the radius factor of the viewing cosine), then
//                    the problem's keypoints stream through LDS in tiles of 256, 64 bytes each.  Level and window are tested eight tile entries
//                    at a time without a branch, then the right-column gate, and the 256-bit Hamming distance is evaluated only for the
//                    survivors.  The lane keeps its YGZ_STRACK_TOPK best as sorted keys (distance << 20 | index) in registers (k_proj_search's
//                    min / max ladder with constant indices).  A block whose points are all culled skips the sweep.
// The claim walk, the ratio test and the rotation histogram are serial chains over lists of a few entries: the entry point resolves them on the
// host from the lists it copied back, inside the same call.
// No atomic, no wait for another workgroup, no scratch, no environment switch.  One packed upload, one launch, one copy back, one wait.
#include "ygz_internal.h"
#include "se3_dev.h"
#include "strack_dev.h"                 // StIn, StSetDev, StProbDev and the kernel's prototype: svo.hip launches it too
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "slot_pose_dev.h"              // the rotation bin and the three maxima of the histogram: svo.hip and srk.hip apply the same rule

#define ST_LANES     256
#define ST_TILE      256
#define ST_GROUP     8                  // tile entries whose level and window are tested together
#define ST_IDX_BITS  20                 // key = distance << 20 | keypoint index
#define ST_TAKEN     0x40000000         // the level a taken keypoint, or an entry past the end, is given in LDS: in no level range
#define ST_NO_KEY    0xFFFFFFFFu

static_assert(ST_LANES == ST_DEV_LANES && ST_IDX_BITS == ST_DEV_IDX_BITS && ST_NO_KEY == ST_DEV_NO_KEY, "strack_dev.h states this file's constants");

struct StKp { double kx, ky, ur; int32_t level, pad_; };     // 32 bytes; the descriptor is another 32

struct StPoint { double u, v, ur, r; int level, lo, hi; };

namespace {

// steps 1-4 of tests/strack_ref.c: the reason, and for reason 0 the pixel, the right column, the level, the radius and the level range
__device__ __forceinline__ int st_point(const StSetDev &S, const StProbDev &P, const StIn &in, int i, StPoint *o)
{
    o->u = 0; o->v = 0; o->ur = 0; o->r = 0; o->level = -1; o->lo = 0; o->hi = -1;
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
    if (P.mode == 0) {
        const int lvl = S.pt_level[i];
        o->level = lvl;
        o->r = P.th * (double)(1 << lvl);
        if (P.direction > 0) { o->lo = lvl; o->hi = in.L - 1; }
        else if (P.direction < 0) { o->lo = 0; o->hi = lvl; }
        else { o->lo = lvl - 1; o->hi = lvl + 1; }
    } else {
        const double d = sqrt(x * x + y * y + z * z);
        const double dmax = S.pt_dmax[i], dmin = dmax / (double)(1 << (in.L - 1));
        if (d < 0.8 * dmin || d > 1.2 * dmax) return 4;
        const double *n = S.pt_normal + 3 * (size_t)i;
        const double n0 = n[0], n1 = n[1], n2 = n[2];
        const double nx = R[0] * n0 + R[1] * n1 + R[2] * n2;
        const double ny = R[3] * n0 + R[4] * n1 + R[5] * n2;
        const double nz = R[6] * n0 + R[7] * n1 + R[8] * n2;
        const double c = x * nx + y * ny + z * nz;
        if (c < 0.5 * d) return 5;
        const double ratio = dmax / d;
        int pred = in.L - 1;
        for (int m = in.L - 2; m >= 0; --m)
            if (ratio <= (double)(1 << m)) pred = m;
        const double f = (c > in.cos_near * d) ? in.r_near : in.r_wide;
        o->level = pred;
        o->r = (P.th * f) * (double)(1 << pred);
        o->lo = pred - 1; o->hi = pred;
    }
    o->u = u; o->v = v; o->ur = u - in.bf * iz;
    return 0;
}

}  // namespace

__global__ __launch_bounds__(ST_LANES) void k_strack_search(const StIn *__restrict__ in_, const StSetDev *__restrict__ sets,
                                                            const StProbDev *__restrict__ probs, uint32_t *__restrict__ keys,
                                                            int32_t *__restrict__ n_cand, int32_t *__restrict__ n_gated,
                                                            int32_t *__restrict__ level, int32_t *__restrict__ reason, double *__restrict__ proj)
{
    __shared__ StKp s_k[ST_TILE];
    __shared__ uint4 s_d[ST_TILE][2];
    const StProbDev &P = probs[blockIdx.y];
    const StSetDev &S = sets[P.set];
    const int n_pt = S.n_pt;
    if ((int)(blockIdx.x * ST_LANES) >= n_pt) return;              // the same in every lane of the block
    const StIn in = *in_;
    const int i = blockIdx.x * ST_LANES + threadIdx.x;
    const bool live = i < n_pt;
    StPoint pt;
    pt.u = 0; pt.v = 0; pt.ur = 0; pt.r = 0; pt.level = -1; pt.lo = 0; pt.hi = -1;
    const int why = live ? st_point(S, P, in, i, &pt) : 1;
    const bool search = live && why == 0;
    uint32_t key[YGZ_STRACK_TOPK];
#pragma unroll
    for (int m = 0; m < YGZ_STRACK_TOPK; ++m) key[m] = ST_NO_KEY;
    int nc = 0, ng = 0;
    if (__syncthreads_or(search)) {
        uint32_t d[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (search) {
            const uint4 a = *reinterpret_cast<const uint4 *>(S.pt_desc + 8 * (size_t)i), b = *reinterpret_cast<const uint4 *>(S.pt_desc + 8 * (size_t)i + 4);
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
        }
        const double u = pt.u, v = pt.v, ur = pt.ur, rad = pt.r;
        const int lo = pt.lo, hi = pt.hi;
        const int n_kp = P.n_kp;
        for (int j0 = 0; j0 < n_kp; j0 += ST_TILE) {
            const int j = j0 + (int)threadIdx.x;
            __syncthreads();
            if (j >= n_kp) s_k[threadIdx.x].level = (int32_t)ST_TAKEN;     // past the end: in no range (the sweep goes in groups of ST_GROUP)
            else {
                StKp k;
                k.kx = P.kp_px[2 * (size_t)j]; k.ky = P.kp_px[2 * (size_t)j + 1];
                k.ur = P.kp_ur ? P.kp_ur[j] : -1.0;
                k.level = (P.kp_taken && P.kp_taken[j]) ? (int32_t)ST_TAKEN : P.kp_level[j];
                k.pad_ = 0;
                s_k[threadIdx.x] = k;
                s_d[threadIdx.x][0] = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j);
                s_d[threadIdx.x][1] = *reinterpret_cast<const uint4 *>(P.kp_desc + 8 * (size_t)j + 4);
            }
            __syncthreads();
            if (!search) continue;
            const int cnt = min(ST_TILE, n_kp - j0);
            // level and window of ST_GROUP entries at a time, without a branch: their LDS reads (one address for all lanes: broadcasts) are in
            // flight together; the gate and the Hamming distance only for the entries whose bit is set, in index order
            for (int t0 = 0; t0 < cnt; t0 += ST_GROUP) {
                uint32_t in_window = 0;
                int glv[ST_GROUP];
                double gx[ST_GROUP], gy[ST_GROUP];
#pragma unroll
                for (int g = 0; g < ST_GROUP; ++g) { glv[g] = s_k[t0 + g].level; gx[g] = s_k[t0 + g].kx; gy[g] = s_k[t0 + g].ky; }
#pragma unroll
                for (int g = 0; g < ST_GROUP; ++g) {
                    const int lv = glv[g];
                    const double dx = gx[g] - u, dy = gy[g] - v;
                    const uint32_t ok = (uint32_t)(lv >= lo) & (uint32_t)(lv <= hi) & (uint32_t)(dx < rad) & (uint32_t)(dx > -rad) &
                                        (uint32_t)(dy < rad) & (uint32_t)(dy > -rad);
                    in_window |= ok << g;
                }
                while (in_window) {
                    const int t = t0 + __ffs((int)in_window) - 1;
                    in_window &= in_window - 1;
                    const double kur = s_k[t].ur;
                    if (kur >= 0) {
                        const double er = ur - kur;
                        if (er > rad || er < -rad) { ++ng; continue; }
                    }
                    const uint4 a = s_d[t][0], b = s_d[t][1];
                    const int dist = __popc(d[0] ^ a.x) + __popc(d[1] ^ a.y) + __popc(d[2] ^ a.z) + __popc(d[3] ^ a.w) +
                                     __popc(d[4] ^ b.x) + __popc(d[5] ^ b.y) + __popc(d[6] ^ b.z) + __popc(d[7] ^ b.w);
                    ++nc;
                    uint32_t k = ((uint32_t)dist << ST_IDX_BITS) | (uint32_t)(j0 + t);
#pragma unroll
                    for (int m = 0; m < YGZ_STRACK_TOPK; ++m) { const uint32_t l = min(key[m], k); k = max(key[m], k); key[m] = l; }
                }
            }
        }
    }
    if (!live) return;
    const size_t g = (size_t)P.pt_off + (size_t)i;
    uint4 *o = reinterpret_cast<uint4 *>(keys + YGZ_STRACK_TOPK * g);
    o[0] = make_uint4(key[0], key[1], key[2], key[3]);
    o[1] = make_uint4(key[4], key[5], key[6], key[7]);
    n_cand[g] = nc;
    n_gated[g] = ng;
    level[g] = pt.level;
    reason[g] = why;
    proj[3 * g] = pt.u; proj[3 * g + 1] = pt.v; proj[3 * g + 2] = pt.ur;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// steps 8 and 9 of tests/strack_ref.c over one problem's lists: the claim walk, then the rotation histogram.  counts [4], rot [33]
static void strack_resolve(const ygz_strack_points &S, const ygz_strack_problem &B, const ygz_strack_params &p, const uint32_t *keys,
                           const int32_t *n_cand, const int32_t *why, int32_t *m_, int32_t *d_, int32_t *oc, int32_t *counts, int32_t *rot,
                           std::vector<uint8_t> &taken, std::vector<int32_t> &bin_)
{
    const int n = S.n_pt;
    const uint32_t idx_mask = (1u << ST_IDX_BITS) - 1;
    taken.assign((size_t)B.n_kp, 0);
    if (B.kp_taken) memcpy(taken.data(), B.kp_taken, (size_t)B.n_kp);
    int nm = 0, ns = 0, nov = 0, nrot = 0;
    for (int i = 0; i < n; ++i) {
        m_[i] = -1; d_[i] = -1; oc[i] = -1;
        if (why[i] != 0) continue;
        ++ns;
        if (n_cand[i] > YGZ_STRACK_TOPK) ++nov;
        const int len = n_cand[i] < YGZ_STRACK_TOPK ? n_cand[i] : YGZ_STRACK_TOPK;
        const uint32_t *k = keys + (size_t)YGZ_STRACK_TOPK * i;
        int e1 = -1, e2 = -1;
        for (int e = 0; e < len; ++e) {
            if (taken[k[e] & idx_mask]) continue;
            if (e1 < 0) e1 = e; else { e2 = e; break; }
        }
        if (e1 < 0) { oc[i] = 1; continue; }
        const int j1 = (int)(k[e1] & idx_mask), d1 = (int)(k[e1] >> ST_IDX_BITS);
        if (d1 > p.th_dist) { oc[i] = 2; continue; }
        if (B.mode == 1 && e2 >= 0) {
            const int j2 = (int)(k[e2] & idx_mask), d2 = (int)(k[e2] >> ST_IDX_BITS);
            if (B.kp_level[j1] == B.kp_level[j2] && (double)d1 > p.ratio * (double)d2) { oc[i] = 3; continue; }
        }
        oc[i] = 0; m_[i] = j1; d_[i] = d1; taken[(size_t)j1] = 1;
    }
    int32_t hist[30], ind[3] = { -1, -1, -1 };
    for (int b = 0; b < 30; ++b) hist[b] = 0;
    if (B.mode == 0 && S.pt_angle && p.check_orientation) {
        bin_.assign((size_t)n, -1);
        for (int i = 0; i < n; ++i) {
            if (m_[i] < 0) continue;
            const int bin = ygz_rot_bin_of((float)(S.pt_angle[i] - B.kp_angle[m_[i]]));      // the host angles are doubles
            if (bin < 0) continue;
            bin_[(size_t)i] = bin;
            hist[bin]++;
        }
        ygz_rot_top3(hist, ind);
        for (int i = 0; i < n; ++i) {
            if (m_[i] < 0) continue;
            const int b = bin_[(size_t)i];
            if (b >= 0 && (b == ind[0] || b == ind[1] || b == ind[2])) continue;
            m_[i] = -1; d_[i] = -1; oc[i] = 4; ++nrot;
        }
    }
    for (int i = 0; i < n; ++i) if (m_[i] >= 0) ++nm;
    if (counts) { counts[0] = nm; counts[1] = ns; counts[2] = nov; counts[3] = nrot; }
    if (rot) { for (int b = 0; b < 30; ++b) rot[b] = hist[b]; rot[30] = ind[0]; rot[31] = ind[1]; rot[32] = ind[2]; }
}

extern "C" {

void ygz_hip_default_strack_params(ygz_strack_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->ratio = 0.8; p->r_near = 2.5; p->r_wide = 4.0; p->cos_near = 0.998; p->th_dist = 100; p->check_orientation = 1;
}

int ygz_hip_stereo_track_search(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_problems, const ygz_strack_problem *problems,
                                const double K4[4], const ygz_strack_params *params, int32_t *match, int32_t *dist, int32_t *level,
                                int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj, int32_t *cand,
                                int32_t *counts, int32_t *rot)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!sets || !problems || !K4 || n_sets < 1 || n_problems < 1) return YGZ_E_INVALID;
    if (n_sets > YGZ_STRACK_MAX_SETS || n_problems > YGZ_STRACK_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    for (int s = 0; s < n_sets; ++s) {
        if (sets[s].n_pt < 0) return YGZ_E_INVALID;
        if (sets[s].n_pt > 0 && (!sets[s].pw || !sets[s].pt_desc)) return YGZ_E_INVALID;
    }
    size_t N = 0;
    bool big = false;
    int max_pt = 0;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_problem &b = problems[q];
        if (b.set < 0 || b.set >= n_sets || b.n_kp < 1 || !b.kp_px || !b.kp_level || !b.kp_desc) return YGZ_E_INVALID;
        if (b.mode < 0 || b.mode > 1 || b.direction < -1 || b.direction > 1) return YGZ_E_INVALID;
        if (!isfinite(b.th) || !(b.th > 0)) return YGZ_E_INVALID;
        const ygz_strack_points &S = sets[b.set];
        if (b.mode == 0) {
            if (S.n_pt > 0 && !S.pt_level) return YGZ_E_INVALID;
            if (S.pt_angle && !b.kp_angle) return YGZ_E_INVALID;
        } else if (S.n_pt > 0 && (!S.pt_dmax || !S.pt_normal)) return YGZ_E_INVALID;
        big = big || b.n_kp > (1 << ST_IDX_BITS);
        N += (size_t)S.n_pt;
        if (S.n_pt > max_pt) max_pt = S.n_pt;
    }
    if (big || N > YGZ_STRACK_MAX_PAIRS) return YGZ_E_CAPACITY;
    ygz_strack_params p;
    if (params) p = *params; else ygz_hip_default_strack_params(&p);
    if (!isfinite(p.baseline) || !isfinite(p.ratio) || !isfinite(p.r_near) || !isfinite(p.r_wide) || !isfinite(p.cos_near)) return YGZ_E_INVALID;
    if (!(p.baseline > 0) || !(p.ratio > 0) || !(p.r_near > 0) || !(p.r_wide > 0) || p.th_dist < 0 || p.th_dist > 256) return YGZ_E_INVALID;
    if (!ygz_all_finite(K4, 4) || !(K4[0] > 0) || !(K4[1] > 0)) return YGZ_E_INVALID;
    for (int s = 0; s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        if (!n) continue;
        if (!ygz_all_finite(sets[s].pw, 3 * n)) return YGZ_E_INVALID;
        if (sets[s].pt_dmax && !ygz_all_finite(sets[s].pt_dmax, n)) return YGZ_E_INVALID;
        if (sets[s].pt_normal && !ygz_all_finite(sets[s].pt_normal, 3 * n)) return YGZ_E_INVALID;
        if (sets[s].pt_angle && !ygz_all_finite(sets[s].pt_angle, n)) return YGZ_E_INVALID;
    }
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_problem &b = problems[q];
        if (!ygz_all_finite(b.T, 7)) return YGZ_E_INVALID;
        if (b.kp_ur && !ygz_all_finite(b.kp_ur, (size_t)b.n_kp)) return YGZ_E_INVALID;
        if (b.kp_angle && !ygz_all_finite(b.kp_angle, (size_t)b.n_kp)) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_problem &b = problems[q];
        if (b.n_kp > ctx->cells) return YGZ_E_CAPACITY;
        for (int j = 0; j < b.n_kp; ++j)
            if (b.kp_level[j] < 0 || b.kp_level[j] >= L) return YGZ_E_INVALID;
        if (b.mode == 0)
            for (int i = 0; i < sets[b.set].n_pt; ++i)
                if (sets[b.set].pt_level[i] < 0 || sets[b.set].pt_level[i] >= L) return YGZ_E_INVALID;
    }
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (counts) memset(counts, 0, (size_t)n_problems * 4 * sizeof(int32_t));
    if (rot)
        for (int q = 0; q < n_problems; ++q) {
            memset(rot + 33 * (size_t)q, 0, 30 * sizeof(int32_t));
            rot[33 * (size_t)q + 30] = rot[33 * (size_t)q + 31] = rot[33 * (size_t)q + 32] = -1;
        }
    if (N == 0) return YGZ_OK;                                      // nothing to search: no launch

    // up: [in | sets | problems | every set's arrays | every problem's arrays), back: [keys | n_cand | n_gated | level | reason | proj)
    const size_t Q = (size_t)n_problems;
    YgzBlobLayout B;
    const size_t o_in = B.add(sizeof(StIn)), o_sets = B.add_n<StSetDev>((size_t)n_sets), o_pb = B.add_n<StProbDev>(Q);
    struct SetOffs { size_t pw, desc, level, dmax, normal; };
    struct ProbOffs { size_t px, level, desc, ur, taken, skip; };
    SetOffs so[YGZ_STRACK_MAX_SETS];
    ProbOffs po[YGZ_STRACK_MAX_PROBLEMS];
    for (int s = 0; s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        so[s].pw = B.add_n<double>(n * 3);
        so[s].desc = B.add_n<uint4>(n * 2);                        // 16-byte aligned: read as two uint4
        so[s].level = B.add_n<int32_t>(sets[s].pt_level ? n : 0);  // the optional arrays take no room when absent
        so[s].dmax = B.add_n<double>(sets[s].pt_dmax ? n : 0);
        so[s].normal = B.add_n<double>(sets[s].pt_normal ? n * 3 : 0);
    }
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_problem &b = problems[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)sets[b.set].n_pt;
        po[q].px = B.add_n<double>(nk * 2);
        po[q].level = B.add_n<int32_t>(nk);
        po[q].desc = B.add_n<uint4>(nk * 2);
        po[q].ur = B.add_n<double>(b.kp_ur ? nk : 0);
        po[q].taken = B.add(b.kp_taken ? nk : 0);
        po[q].skip = B.add(b.pt_skip ? np : 0);
    }
    const size_t in_end = B.end;
    const size_t o_keys = B.add_n<uint4>(N * 2), o_nc = B.add_n<int32_t>(N), o_ng = B.add_n<int32_t>(N), o_lvl = B.add_n<int32_t>(N);
    const size_t o_why = B.add_n<int32_t>(N), o_proj = B.add_n<double>(N * 3), total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_STRACK, total, total, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    StIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.bf = K4[0] * p.baseline; in.r_near = p.r_near; in.r_wide = p.r_wide; in.cos_near = p.cos_near;
    in.w = ctx->prm.image_width; in.h = ctx->prm.image_height; in.L = L;
    memcpy(up + o_in, &in, sizeof in);
    for (int s = 0; s < n_sets; ++s) {
        const ygz_strack_points &b = sets[s];
        const size_t n = (size_t)b.n_pt;
        StSetDev D;
        memset(&D, 0, sizeof D);
        if (n) {
            memcpy(up + so[s].pw, b.pw, n * 24); memcpy(up + so[s].desc, b.pt_desc, n * 32);
            if (b.pt_level) memcpy(up + so[s].level, b.pt_level, n * 4);
            if (b.pt_dmax) memcpy(up + so[s].dmax, b.pt_dmax, n * 8);
            if (b.pt_normal) memcpy(up + so[s].normal, b.pt_normal, n * 24);
        }
        D.pw = ygz_at<const double>(dev, so[s].pw); D.pt_desc = ygz_at<const uint32_t>(dev, so[s].desc);
        D.pt_level = b.pt_level ? ygz_at<const int32_t>(dev, so[s].level) : nullptr;
        D.pt_dmax = b.pt_dmax ? ygz_at<const double>(dev, so[s].dmax) : nullptr;
        D.pt_normal = b.pt_normal ? ygz_at<const double>(dev, so[s].normal) : nullptr;
        D.n_pt = b.n_pt;
        memcpy(up + o_sets + (size_t)s * sizeof(StSetDev), &D, sizeof D);
    }
    std::vector<size_t> offs(Q + 1, 0);
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_problem &b = problems[q];
        const size_t nk = (size_t)b.n_kp, np = (size_t)sets[b.set].n_pt;
        memcpy(up + po[q].px, b.kp_px, nk * 16); memcpy(up + po[q].level, b.kp_level, nk * 4); memcpy(up + po[q].desc, b.kp_desc, nk * 32);
        if (b.kp_ur) memcpy(up + po[q].ur, b.kp_ur, nk * 8);
        if (b.kp_taken) memcpy(up + po[q].taken, b.kp_taken, nk);
        if (b.pt_skip && np) memcpy(up + po[q].skip, b.pt_skip, np);
        StProbDev D;
        memset(&D, 0, sizeof D);
        D.kp_px = ygz_at<const double>(dev, po[q].px); D.kp_level = ygz_at<const int32_t>(dev, po[q].level);
        D.kp_desc = ygz_at<const uint32_t>(dev, po[q].desc); D.kp_ur = b.kp_ur ? ygz_at<const double>(dev, po[q].ur) : nullptr;
        D.kp_taken = b.kp_taken ? dev + po[q].taken : nullptr; D.pt_skip = b.pt_skip ? dev + po[q].skip : nullptr;
        D.n_kp = b.n_kp; D.set = b.set; D.pt_off = (int32_t)offs[q]; D.mode = b.mode; D.direction = b.direction; D.th = b.th;
        for (int k = 0; k < 7; ++k) D.T[k] = b.T[k];
        memcpy(up + o_pb + (size_t)q * sizeof(StProbDev), &D, sizeof D);
        offs[q + 1] = offs[q] + np;
    }
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;
    YGZ_LAUNCH(ctx, KID_STRACK_SEARCH, k_strack_search, dim3((unsigned)ygz_div_up(max_pt, ST_LANES), (unsigned)n_problems), dim3(ST_LANES),
               ygz_at<const StIn>(dev, o_in), ygz_at<const StSetDev>(dev, o_sets), ygz_at<const StProbDev>(dev, o_pb), ygz_at<uint32_t>(dev, o_keys),
               ygz_at<int32_t>(dev, o_nc), ygz_at<int32_t>(dev, o_ng), ygz_at<int32_t>(dev, o_lvl), ygz_at<int32_t>(dev, o_why),
               ygz_at<double>(dev, o_proj));
    if ((rc = ygz_blob_fetch(ctx, blob, o_keys, total)) != YGZ_OK) return rc;
    const uint32_t *keys = ygz_at<const uint32_t>(up, o_keys);
    const int32_t *nc = ygz_at<const int32_t>(up, o_nc), *why = ygz_at<const int32_t>(up, o_why);
    if (n_cand) memcpy(n_cand, nc, N * 4);
    if (n_gated) memcpy(n_gated, up + o_ng, N * 4);
    if (level) memcpy(level, up + o_lvl, N * 4);
    if (reason) memcpy(reason, why, N * 4);
    if (proj) memcpy(proj, up + o_proj, N * 24);
    if (cand)
        for (size_t g = 0; g < N * YGZ_STRACK_TOPK; ++g) cand[g] = keys[g] == ST_NO_KEY ? -1 : (int32_t)(keys[g] & ((1u << ST_IDX_BITS) - 1));
    std::vector<int32_t> m_((size_t)max_pt), d_((size_t)max_pt), oc((size_t)max_pt), bin_;
    std::vector<uint8_t> taken;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_strack_points &S = sets[problems[q].set];
        const size_t o = offs[q], n = (size_t)S.n_pt;
        strack_resolve(S, problems[q], p, keys + YGZ_STRACK_TOPK * o, nc + o, why + o, m_.data(), d_.data(), oc.data(),
                       counts ? counts + 4 * (size_t)q : nullptr, rot ? rot + 33 * (size_t)q : nullptr, taken, bin_);
        if (match && n) memcpy(match + o, m_.data(), n * 4);
        if (dist && n) memcpy(dist + o, d_.data(), n * 4);
        if (outcome && n) memcpy(outcome + o, oc.data(), n * 4);
    }
    return YGZ_OK;
}

}  // extern "C"
