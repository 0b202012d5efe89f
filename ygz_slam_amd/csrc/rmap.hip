// The resident map: the map of ygz_hip_local_map_select, ygz_hip_map_point_attributes and
// ygz_hip_stereo_local_map_indexed with a home in device memory, and local-map tracking on it in ONE call.  The kernels of those three calls
// are launched from their own files (ygz_lms_launch, ygz_mpa_launch, ygz_slm_launch_index, ygz_slm_run); this file adds the map object, the
// delta and what stands between the selection and the tracking:
//   k_rmap_filter   one workgroup per frame.  It walks the frame's selected list 256 entries at a time; an entry stays when its point has
//                   state 1 and a descriptor.  The kept ones are compacted in order by a wave ballot and a prefix over the four waves' counts in
//                   wave order: no atomic, and the result does not depend on the order the lanes arrive in.  It writes the filtered list (padded
//                   with -1), moved, the two counts, and the list's length into the table k_slm_index and k_slm_gather read, and zeroes the
//                   list's skip bytes.  Behind a barrier the same workgroup writes the frame's prior row: moved[] of the selection's fr_prior.
//   k_rmap_scatter  a lane per row of a delta: point rows (position, descriptor, bad flag, descriptor flag, each optional), keyframe rows
//                   (bad flag), centre rows.  Indices are distinct within an array, so no two lanes write one address.
// Integers and copies only: no floating-point arithmetic, no atomic, no wait for another workgroup, no scratch memory, no environment
// switch; every loop is a `for` over a count known at entry and every index a kernel forms was validated by an entry point or by the launch
// that wrote it.
#include "ygz_internal.h"
#include "rmap_host.h"
#include "lms_dev.h"
#include "mpa_dev.h"
#include "slm_share.h"
#include <algorithm>
#include <string.h>
#pragma clang fp contract(off)

// a growable buffer of the map's own: ygz_scratch's rule, and the stream is waited for before memory a launch may still read is freed
struct RmapBuf { uint8_t *p = nullptr; size_t bytes = 0; };

struct ygz_hip_map {
    ygz_hip_ctx *ctx = nullptr;
    RmapBuf store, work;                             // the map; the rows of a delta or the selection side of a tracking call
    uint8_t *work_host = nullptr; size_t work_host_bytes = 0;   // page-locked image of `work`
    int K = 0, C = 0, P = 0, N = 0, Kc = 0, R = 0;   // keyframes, covisible columns, points, observations, centres, attribute rows
    int uploads = 0, updates = 0;
    bool valid = false;
};

namespace {

#define RM_LANES 256
#define RM_WAVES (RM_LANES / 64)

struct RmapFilterDev {
    int max_pt, cells;
    const int32_t *state; const uint8_t *has_desc;
    const int32_t *n_pt0, *local_pt0, *fr_off, *fr_prior;    // the selection's n_pt, local_pt [F][max_pt], the frames' offsets, fr_prior
    int32_t *n_pt, *n_removed, *local_pt, *moved, *prior;    // [F], [F], [F][max_pt], [F][max_pt], [F][cells]
    SlmSetTab *tab;                                          // [F]
    uint8_t *pt_skip;                                        // [F][max_pt]
};

__global__ __launch_bounds__(RM_LANES) void k_rmap_filter(RmapFilterDev A)
{
    __shared__ int32_t s_w[RM_WAVES];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, lane = ygz_lane(), wave = tid >> 6;
    const int n0 = min(max(A.n_pt0[f], 0), A.max_pt);
    const size_t row = (size_t)f * (size_t)A.max_pt;
    int run = 0;
    for (int c0 = 0; c0 < n0; c0 += RM_LANES) {
        const int i = c0 + tid;
        int p = -1;
        bool keep = false;
        if (i < n0) {
            p = A.local_pt0[row + i];
            keep = p >= 0 && A.state[p] == 1 && A.has_desc[p] != 0;
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < RM_WAVES; ++w) { const int c = s_w[w]; off += w < wave ? c : 0; tot += c; }
        __syncthreads();
        const int pos = run + off + __popcll(b & ((1ull << lane) - 1ull));
        if (i < n0) A.moved[row + i] = keep ? pos : -1;
        if (keep) A.local_pt[row + pos] = p;                              // pos <= i < max_pt
        run += tot;
    }
    for (int i = run + tid; i < A.max_pt; i += RM_LANES) A.local_pt[row + i] = -1;
    for (int i = tid; i < run; i += RM_LANES) A.pt_skip[row + i] = 0;
    if (tid == 0) { A.n_pt[f] = run; A.n_removed[f] = n0 - run; A.tab[f].n_pt = run; }
    __syncthreads();                                                      // moved, as this workgroup's lanes left it
    const int e0 = A.fr_off[f], n_ent = A.fr_off[f + 1] - e0;
    for (int j = tid; j < A.cells; j += RM_LANES) {
        const int at = j < n_ent ? A.fr_prior[e0 + j] : -1;
        A.prior[(size_t)f * (size_t)A.cells + j] = (at >= 0 && at < n0) ? A.moved[row + at] : -1;
    }
}

struct RmapScatterDev {
    int n_pt, n_kf, n_c;
    const int32_t *pt_idx, *kf_idx, *c_idx;
    const double *r_pw, *r_centre; const uint4 *r_desc; const uint8_t *r_pbad, *r_has, *r_kbad;   // the rows; a null array keeps
    double *pw, *centre; uint4 *desc; uint8_t *pt_bad, *has_desc, *kf_bad;                           // the map
};

__global__ __launch_bounds__(RM_LANES) void k_rmap_scatter(RmapScatterDev A)
{
    int i = (int)blockIdx.x * RM_LANES + (int)threadIdx.x;
    if (i < A.n_pt) {
        const size_t p = (size_t)A.pt_idx[i], r = (size_t)i;
        if (A.r_pw) { A.pw[3 * p] = A.r_pw[3 * r]; A.pw[3 * p + 1] = A.r_pw[3 * r + 1]; A.pw[3 * p + 2] = A.r_pw[3 * r + 2]; }
        if (A.r_desc) { A.desc[2 * p] = A.r_desc[2 * r]; A.desc[2 * p + 1] = A.r_desc[2 * r + 1]; }
        if (A.r_pbad) A.pt_bad[p] = A.r_pbad[r];
        if (A.r_has) A.has_desc[p] = A.r_has[r];
        return;
    }
    i -= A.n_pt;
    if (i < A.n_kf) { A.kf_bad[A.kf_idx[i]] = A.r_kbad[i]; return; }
    i -= A.n_kf;
    if (i < A.n_c) {
        const size_t c = (size_t)A.c_idx[i], r = (size_t)i;
        A.centre[3 * c] = A.r_centre[3 * r]; A.centre[3 * c + 1] = A.r_centre[3 * r + 1]; A.centre[3 * c + 2] = A.r_centre[3 * r + 2];
    }
}

int buf_fit(ygz_hip_ctx *ctx, RmapBuf &b, size_t bytes)
{
    if (b.bytes >= bytes) return YGZ_OK;
    if (b.p) { YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    const size_t cap = ygz_rmap_grown(bytes);
    YGZ_HIPCHK(ctx, hipMalloc((void **)&b.p, cap));
    b.bytes = cap;
    return YGZ_OK;
}

// the work buffer with its page-locked image, both of at least `bytes`
int work_fit(ygz_hip_ctx *ctx, ygz_hip_map *m, size_t bytes)
{
    const int rc = buf_fit(ctx, m->work, bytes);
    if (rc != YGZ_OK) return rc;
    if (m->work_host_bytes >= m->work.bytes) return YGZ_OK;
    if (m->work_host) { YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipHostFree(m->work_host); m->work_host = nullptr; m->work_host_bytes = 0; }
    YGZ_HIPCHK(ctx, hipHostMalloc((void **)&m->work_host, m->work.bytes, hipHostMallocDefault));
    m->work_host_bytes = m->work.bytes;
    return YGZ_OK;
}

bool map_ok(const ygz_hip_ctx *ctx, const ygz_hip_map *m)
{
    // by address alone: a handle the context does not know (another context's, a destroyed one) is never dereferenced
    return m && std::find(ctx->maps.begin(), ctx->maps.end(), m) != ctx->maps.end();
}

RmapStore store_of(const ygz_hip_map *m)
{
    return RmapStore((size_t)m->K, (size_t)m->C, (size_t)m->P, (size_t)m->N, (size_t)m->Kc, (size_t)m->R);
}

void attr_launch(ygz_hip_ctx *ctx, const ygz_hip_map *m, const RmapStore &S)
{
    MpaDev A;
    A.P = m->P;
    A.center = ygz_at<const double>(m->store.p, S.o_centre); A.pw = ygz_at<const double>(m->store.p, S.o_pw);
    A.offsets = ygz_at<const int32_t>(m->store.p, S.o_aoff); A.obs_kf = ygz_at<const int32_t>(m->store.p, S.o_akf);
    A.obs_level = ygz_at<const int32_t>(m->store.p, S.o_alv);
    A.dmax = ygz_at<double>(m->store.p, S.o_dmax); A.normal = ygz_at<double>(m->store.p, S.o_nrm); A.state = ygz_at<int32_t>(m->store.p, S.o_state);
    ygz_mpa_launch(ctx, A);
}

void map_free(ygz_hip_map *m)
{
    if (m->store.p) (void)hipFree(m->store.p);
    if (m->work.p) (void)hipFree(m->work.p);
    if (m->work_host) (void)hipHostFree(m->work_host);
    delete m;
}

// ---- the resident source of ygz_slm_run: everything between the tracking block's upload and k_slm_index
struct ResidentCall {
    ygz_hip_map *map;
    int n_frames, n_ent, max_len;
    const int32_t *fr_off, *fr_pt;
    ygz_lms_params q;
    bool want_votes, want_prior;
    RmapCall L;
    ResidentCall(size_t F, size_t K, size_t E, size_t MP, size_t cells) : L(F, K, E, MP, cells) {}
};

int resident_hook(ygz_hip_ctx *ctx, void *user, SlmResidentDev &R)
{
    ResidentCall &c = *static_cast<ResidentCall *>(user);
    ygz_hip_map *m = c.map;
    const RmapCall &L = c.L;
    if (L.bad) return YGZ_E_CAPACITY;
    int rc = work_fit(ctx, m, L.end);
    if (rc != YGZ_OK) return rc;
    uint8_t *host = m->work_host, *dev = m->work.p;
    const size_t F = (size_t)c.n_frames, E = (size_t)c.n_ent;
    memcpy(host + L.o_foff, c.fr_off, (F + 1) * 4);
    if (E) memcpy(host + L.o_fpt, c.fr_pt, E * 4);
    YGZ_HIPCHK(ctx, hipMemcpyAsync(dev, host, L.in_end, hipMemcpyHostToDevice, ctx->stream));
    const RmapStore S = store_of(m);
    uint8_t *st = m->store.p;
    LmsDev A;
    A.K = m->K; A.C = m->C; A.max_kf = c.q.max_keyframes; A.max_pt = c.q.max_points;
    A.kf_bad = st + S.o_kbad; A.pt_bad = st + S.o_pbad;
    A.cov = ygz_at<const int32_t>(st, S.o_cov); A.offsets = ygz_at<const int32_t>(st, S.o_off); A.obs = ygz_at<const int32_t>(st, S.o_obs);
    A.koff = ygz_at<const int32_t>(st, S.o_koff); A.kpt = ygz_at<const int32_t>(st, S.o_kpt);
    A.fr_off = ygz_at<const int32_t>(dev, L.o_foff); A.fr_pt = ygz_at<const int32_t>(dev, L.o_fpt);
    A.votes = ygz_at<int32_t>(dev, L.o_votes); A.ref = ygz_at<int32_t>(dev, L.o_ref); A.n_voters = ygz_at<int32_t>(dev, L.o_nvot);
    A.n_local = ygz_at<int32_t>(dev, L.o_nloc); A.local_kf = ygz_at<int32_t>(dev, L.o_lkf); A.n_pt = ygz_at<int32_t>(dev, L.o_npt0);
    A.n_cut = ygz_at<int32_t>(dev, L.o_ncut); A.local_pt = ygz_at<int32_t>(dev, L.o_lpt0); A.fr_prior = ygz_at<int32_t>(dev, L.o_fprior);
    A.rank = ygz_at<uint16_t>(dev, L.o_rank); A.cnt = ygz_at<int32_t>(dev, L.o_cnt); A.start = ygz_at<int32_t>(dev, L.o_start);
    A.local_ft = ygz_at<int32_t>(dev, L.o_lft);
    ygz_lms_launch(ctx, A, c.n_frames, c.max_len);
    RmapFilterDev G;
    G.max_pt = c.q.max_points; G.cells = R.cells;
    G.state = ygz_at<const int32_t>(st, S.o_state); G.has_desc = st + S.o_has;
    G.n_pt0 = A.n_pt; G.local_pt0 = A.local_pt; G.fr_off = A.fr_off; G.fr_prior = A.fr_prior;
    G.n_pt = ygz_at<int32_t>(dev, L.o_npt); G.n_removed = ygz_at<int32_t>(dev, L.o_nrem); G.local_pt = ygz_at<int32_t>(dev, L.o_lpt);
    G.moved = ygz_at<int32_t>(dev, L.o_moved); G.prior = ygz_at<int32_t>(dev, L.o_prior);
    G.tab = R.tab; G.pt_skip = R.pt_skip;
    YGZ_LAUNCH(ctx, KID_RMAP_FILTER, k_rmap_filter, dim3((unsigned)c.n_frames), dim3(RM_LANES), G);
    // the selection's outputs start their way back now; the tracking block's copy back waits for both
    const size_t back = L.back_end(c.want_votes, c.want_prior);
    YGZ_HIPCHK(ctx, hipMemcpyAsync(host + L.o_ref, dev + L.o_ref, back - L.o_ref, hipMemcpyDeviceToHost, ctx->stream));
    R.list_pt = G.local_pt; R.prior = G.prior;
    return YGZ_OK;
}

// row f of a per-point output: the first n_pt[f] entries, `width` elements each
template <class T> void copy_rows(T *dst, const std::vector<T> &src, const int32_t *n_pt, size_t F, size_t MP, size_t width)
{
    if (!dst) return;
    for (size_t f = 0; f < F; ++f)
        if (n_pt[f] > 0) memcpy(dst + f * MP * width, src.data() + f * MP * width, (size_t)n_pt[f] * width * sizeof(T));
}

}  // namespace

void ygz_rmap_free_all(ygz_hip_ctx *ctx)
{
    for (ygz_hip_map *m : ctx->maps) map_free(m);
    ctx->maps.clear();
}

extern "C" {

int ygz_hip_map_create(ygz_hip_ctx *ctx, ygz_hip_map **map)
{
    if (!map || !ctx) return YGZ_E_INVALID;
    ygz_hip_map *m = new ygz_hip_map;
    m->ctx = ctx;
    ctx->maps.push_back(m);
    *map = m;
    return YGZ_OK;
}

int ygz_hip_map_destroy(ygz_hip_ctx *ctx, ygz_hip_map *map)
{
    if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->maps.erase(std::find(ctx->maps.begin(), ctx->maps.end(), map));
    map_free(map);
    return YGZ_OK;
}

int ygz_hip_map_info(ygz_hip_ctx *ctx, ygz_hip_map *map, ygz_map_info *info)
{
    if (!info || !ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    memset(info, 0, sizeof *info);
    if (map->valid) {
        info->n_keyframes = map->K; info->n_cov = map->C; info->n_points = map->P; info->n_obs = map->N; info->n_centres = map->Kc;
        info->n_rows = map->R;
    }
    info->uploads = map->uploads; info->updates = map->updates;
    info->resident_bytes = (uint64_t)(map->store.bytes + map->work.bytes);
    return YGZ_OK;
}

int ygz_hip_map_upload(ygz_hip_ctx *ctx, ygz_hip_map *map, const ygz_map_arrays *a, double *dmax, double *normal, int32_t *state)
{
    int n_obs = 0, n_rows = 0;
    int rc = ygz_rmap_check_arrays(a, &n_obs, &n_rows);
    if (rc != YGZ_OK) return rc;
    if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    const size_t K = (size_t)a->n_keyframes, C = (size_t)a->n_cov, P = (size_t)a->n_points, N = (size_t)n_obs, Kc = (size_t)a->n_centres,
                 R = (size_t)n_rows;
    const RmapStore S(K, C, P, N, Kc, R);
    if (S.bad) return YGZ_E_CAPACITY;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // the image first: a failure up to here leaves the resident map as it was
    uint8_t *host = (uint8_t *)ygz_stage(ctx, S.end);
    if (!host) return YGZ_E_HIP;
    memcpy(host + S.o_kbad, a->kf_bad, K);
    if (a->pt_bad) memcpy(host + S.o_pbad, a->pt_bad, P); else memset(host + S.o_pbad, 0, P);
    if (a->pt_has_desc) memcpy(host + S.o_has, a->pt_has_desc, P); else memset(host + S.o_has, 1, P);
    if (K * C) memcpy(host + S.o_cov, a->cov, K * C * 4);
    memcpy(host + S.o_off, a->offsets, (P + 1) * 4);
    {
        int32_t *obs = ygz_at<int32_t>(host, S.o_obs);
        for (size_t g = 0; g < N; ++g) obs[g] = a->kf[g] | (a->feat[g] << 16);
    }
    ygz_lms_build_index(a->n_points, a->offsets, a->kf, a->feat, a->n_keyframes, ygz_at<int32_t>(host, S.o_koff), ygz_at<int32_t>(host, S.o_kpt), nullptr);
    memcpy(host + S.o_centre, a->centre, 3 * Kc * 8);
    memcpy(host + S.o_pw, a->pw, 3 * P * 8);
    memcpy(host + S.o_aoff, a->a_offsets, (P + 1) * 4);
    if (R) { memcpy(host + S.o_akf, a->a_kf, R * 4); memcpy(host + S.o_alv, a->a_level, R * 4); }
    memcpy(host + S.o_desc, a->pt_desc, 32 * P);
    if (map->store.bytes < S.end) map->valid = false;                    // the old buffer goes: a failed allocation leaves an empty map
    if ((rc = buf_fit(ctx, map->store, S.end)) != YGZ_OK) return rc;
    map->valid = false;
    YGZ_HIPCHK(ctx, hipMemcpyAsync(map->store.p, host, S.in_end, hipMemcpyHostToDevice, ctx->stream));
    map->K = (int)K; map->C = (int)C; map->P = (int)P; map->N = (int)N; map->Kc = (int)Kc; map->R = (int)R;
    attr_launch(ctx, map, S);
    YGZ_HIPCHK(ctx, hipGetLastError());
    const bool back = dmax || normal || state;
    if (back) YGZ_HIPCHK(ctx, hipMemcpyAsync(host + S.o_dmax, map->store.p + S.o_dmax, S.end - S.o_dmax, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    map->valid = true;
    ++map->uploads;
    if (dmax) memcpy(dmax, host + S.o_dmax, P * 8);
    if (normal) memcpy(normal, host + S.o_nrm, 3 * P * 8);
    if (state) memcpy(state, host + S.o_state, P * 4);
    return YGZ_OK;
}

int ygz_hip_map_update(ygz_hip_ctx *ctx, ygz_hip_map *map, int n_pt, const int32_t *pt_idx, const double *pw, const uint8_t *pt_desc,
                       const uint8_t *pt_bad, const uint8_t *pt_has_desc, int n_kf, const int32_t *kf_idx, const uint8_t *kf_bad, int n_c,
                       const int32_t *c_idx, const double *centre)
{
    if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    if (!map->valid) return YGZ_E_STATE;
    int rc = ygz_rmap_check_delta(map->P, map->K, map->Kc, n_pt, pt_idx, pw, n_kf, kf_idx, kf_bad, n_c, c_idx, centre);
    if (rc != YGZ_OK) return rc;
    const size_t np = (size_t)n_pt, nk = (size_t)n_kf, nc = (size_t)n_c;
    const RmapDelta D(np, pw != nullptr, pt_desc != nullptr, pt_bad != nullptr, pt_has_desc != nullptr, nk, nc);
    if (D.bad) return YGZ_E_CAPACITY;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    if ((rc = work_fit(ctx, map, D.end)) != YGZ_OK) return rc;
    uint8_t *host = map->work_host, *dev = map->work.p;
    if (np) {
        memcpy(host + D.o_pidx, pt_idx, np * 4);
        if (pw) memcpy(host + D.o_pw, pw, np * 24);
        if (pt_desc) memcpy(host + D.o_desc, pt_desc, np * 32);
        if (pt_bad) memcpy(host + D.o_pbad, pt_bad, np);
        if (pt_has_desc) memcpy(host + D.o_has, pt_has_desc, np);
    }
    if (nk) { memcpy(host + D.o_kidx, kf_idx, nk * 4); memcpy(host + D.o_kbad, kf_bad, nk); }
    if (nc) { memcpy(host + D.o_cidx, c_idx, nc * 4); memcpy(host + D.o_centre, centre, nc * 24); }
    const RmapStore S = store_of(map);
    uint8_t *st = map->store.p;
    const size_t rows = np + nk + nc;
    if (rows) {
        YGZ_HIPCHK(ctx, hipMemcpyAsync(dev, host, D.end, hipMemcpyHostToDevice, ctx->stream));
        RmapScatterDev A;
        A.n_pt = n_pt; A.n_kf = n_kf; A.n_c = n_c;
        A.pt_idx = ygz_at<const int32_t>(dev, D.o_pidx); A.kf_idx = ygz_at<const int32_t>(dev, D.o_kidx); A.c_idx = ygz_at<const int32_t>(dev, D.o_cidx);
        A.r_pw = pw ? ygz_at<const double>(dev, D.o_pw) : nullptr; A.r_centre = ygz_at<const double>(dev, D.o_centre);
        A.r_desc = pt_desc ? ygz_at<const uint4>(dev, D.o_desc) : nullptr;
        A.r_pbad = pt_bad ? dev + D.o_pbad : nullptr; A.r_has = pt_has_desc ? dev + D.o_has : nullptr; A.r_kbad = dev + D.o_kbad;
        A.pw = ygz_at<double>(st, S.o_pw); A.centre = ygz_at<double>(st, S.o_centre); A.desc = ygz_at<uint4>(st, S.o_desc);
        A.pt_bad = st + S.o_pbad; A.has_desc = st + S.o_has; A.kf_bad = st + S.o_kbad;
        YGZ_LAUNCH(ctx, KID_RMAP_SCATTER, k_rmap_scatter, dim3((unsigned)((rows + RM_LANES - 1) / RM_LANES)), dim3(RM_LANES), A);
    }
    attr_launch(ctx, map, S);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ++map->updates;
    return YGZ_OK;
}

int ygz_hip_map_download(ygz_hip_ctx *ctx, ygz_hip_map *map, double *pw, uint8_t *pt_desc, uint8_t *pt_bad, uint8_t *pt_has_desc,
                         uint8_t *kf_bad, double *centre, double *dmax, double *normal, int32_t *state)
{
    if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    if (!map->valid) return YGZ_E_STATE;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const RmapStore S = store_of(map);
    uint8_t *host = (uint8_t *)ygz_stage(ctx, S.end);
    if (!host) return YGZ_E_HIP;
    YGZ_HIPCHK(ctx, hipMemcpyAsync(host, map->store.p, S.end, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t P = (size_t)map->P;
    if (pw) memcpy(pw, host + S.o_pw, 3 * P * 8);
    if (pt_desc) memcpy(pt_desc, host + S.o_desc, 32 * P);
    if (pt_bad) memcpy(pt_bad, host + S.o_pbad, P);
    if (pt_has_desc) memcpy(pt_has_desc, host + S.o_has, P);
    if (kf_bad) memcpy(kf_bad, host + S.o_kbad, (size_t)map->K);
    if (centre) memcpy(centre, host + S.o_centre, 3 * (size_t)map->Kc * 8);
    if (dmax) memcpy(dmax, host + S.o_dmax, P * 8);
    if (normal) memcpy(normal, host + S.o_nrm, 3 * P * 8);
    if (state) memcpy(state, host + S.o_state, P * 4);
    return YGZ_OK;
}

int ygz_hip_stereo_local_map_resident(ygz_hip_ctx *ctx, ygz_hip_map *map, int n_frames, const int32_t *slot, const double *T,
                                      const int32_t *fr_off, const int32_t *fr_pt, const ygz_lms_params *lms, const ygz_slm_params *params,
                                      int32_t *votes, int32_t *ref, int32_t *n_voters, int32_t *n_local, int32_t *local_kf, int32_t *n_cut,
                                      int32_t *n_pt, int32_t *local_pt, int32_t *n_removed, int32_t *prior, double *T_out, int32_t *status,
                                      int32_t *counts, int32_t *kp_point, uint8_t *outlier, double *chi2, int32_t *inliers,
                                      int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                      double *round_cost_final, double *round_lambda, int32_t *match, int32_t *dist, int32_t *level,
                                      int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj)
{
    if (!slot || !T || !fr_off || !fr_pt || !T_out || n_frames < 1) return YGZ_E_INVALID;
    if (n_frames > YGZ_LMS_MAX_FRAMES) return YGZ_E_CAPACITY;
    ygz_lms_params q;
    ygz_hip_default_lms_params(&q);
    if (lms) q = *lms;
    if (q.max_keyframes < 1 || q.max_keyframes > YGZ_LMS_MAX_KEYFRAMES || q.max_points < 1) return YGZ_E_INVALID;
    if ((int64_t)n_frames * q.max_points > YGZ_SLM_MAX_PAIRS) return YGZ_E_CAPACITY;
    if (fr_off[0] != 0) return YGZ_E_INVALID;
    int max_len = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (fr_off[f + 1] < fr_off[f]) return YGZ_E_INVALID;
        max_len = std::max(max_len, fr_off[f + 1] - fr_off[f]);
    }
    if (max_len > YGZ_LMS_MAX_FEATURES) return YGZ_E_CAPACITY;
    if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;
    if (!map->valid) return YGZ_E_STATE;
    if ((int64_t)n_frames * map->K > YGZ_COVIS_MAX_CELLS) return YGZ_E_CAPACITY;
    const int n_ent = fr_off[n_frames];
    for (int e = 0; e < n_ent; ++e)
        if (fr_pt[e] < -1 || fr_pt[e] >= map->P) return YGZ_E_INVALID;
    if (max_len > ctx->cells) return YGZ_E_INVALID;
    const size_t F = (size_t)n_frames, K = (size_t)map->K, MP = (size_t)q.max_points, Cn = (size_t)ctx->cells, NP = F * MP;
    ResidentCall call(F, K, (size_t)n_ent, MP, Cn);
    call.map = map; call.n_frames = n_frames; call.n_ent = n_ent; call.max_len = max_len; call.fr_off = fr_off; call.fr_pt = fr_pt; call.q = q;
    call.want_votes = votes != nullptr; call.want_prior = prior != nullptr;
    const RmapStore S = store_of(map);
    SlmSource src;
    src.n_sets = n_frames; src.n_points = map->P; src.stride = q.max_points;
    src.pw = ygz_at<const double>(map->store.p, S.o_pw); src.desc = map->store.p + S.o_desc;
    src.dmax = ygz_at<const double>(map->store.p, S.o_dmax); src.normal = ygz_at<const double>(map->store.p, S.o_nrm);
    src.index = ygz_slm_launch_index; src.resident = resident_hook; src.user = &call;
    // the per-point outputs come back at the stride and are handed on row by row
    std::vector<int32_t> list_of(F), v_match(match ? NP : 0), v_dist(dist ? NP : 0), v_level(level ? NP : 0), v_reason(reason ? NP : 0),
        v_outcome(outcome ? NP : 0), v_ncand(n_cand ? NP : 0), v_ngated(n_gated ? NP : 0);
    std::vector<double> v_proj(proj ? 3 * NP : 0);
    for (size_t f = 0; f < F; ++f) list_of[f] = (int32_t)f;
    // ygz_slm_run writes its outputs behind its one wait, so the other arrays are the caller's own
    const SlmOutputs out = { T_out, status, counts, kp_point, outlier, chi2, inliers, rounds_run, round_status, round_iterations, round_cost_initial,
                             round_cost_final, round_lambda, match ? v_match.data() : nullptr, dist ? v_dist.data() : nullptr,
                             level ? v_level.data() : nullptr, reason ? v_reason.data() : nullptr, outcome ? v_outcome.data() : nullptr,
                             n_cand ? v_ncand.data() : nullptr, n_gated ? v_ngated.data() : nullptr, proj ? v_proj.data() : nullptr };
    const int rc = ygz_slm_run(ctx, src, n_frames, slot, list_of.data(), T, nullptr, params, out);
    if (rc != YGZ_OK) return rc;
    // both copies back have landed
    const uint8_t *host = map->work_host;
    const RmapCall &L = call.L;
    const int32_t *h_npt = ygz_at<const int32_t>(const_cast<uint8_t *>(host), L.o_npt);
    if (votes) memcpy(votes, host + L.o_votes, F * K * 4);
    if (ref) memcpy(ref, host + L.o_ref, F * 4);
    if (n_voters) memcpy(n_voters, host + L.o_nvot, F * 4);
    if (n_local) memcpy(n_local, host + L.o_nloc, F * 4);
    if (local_kf) memcpy(local_kf, host + L.o_lkf, F * K * 4);
    if (n_cut) memcpy(n_cut, host + L.o_ncut, F * 4);
    if (n_pt) memcpy(n_pt, h_npt, F * 4);
    if (local_pt) memcpy(local_pt, host + L.o_lpt, NP * 4);
    if (n_removed) memcpy(n_removed, host + L.o_nrem, F * 4);
    if (prior) memcpy(prior, host + L.o_prior, F * Cn * 4);
    copy_rows(match, v_match, h_npt, F, MP, 1); copy_rows(dist, v_dist, h_npt, F, MP, 1); copy_rows(level, v_level, h_npt, F, MP, 1);
    copy_rows(reason, v_reason, h_npt, F, MP, 1); copy_rows(outcome, v_outcome, h_npt, F, MP, 1); copy_rows(n_cand, v_ncand, h_npt, F, MP, 1);
    copy_rows(n_gated, v_ngated, h_npt, F, MP, 1); copy_rows(proj, v_proj, h_npt, F, MP, 3);
    return YGZ_OK;
}

}  // extern "C"
