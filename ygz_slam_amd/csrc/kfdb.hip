// Keyframe database: the BoW vectors of the map's keyframes resident in HBM, and the place-recognition query that starts relocalisation and
// loop detection.  Nothing in the reference; ORB-SLAM2's KeyFrameDatabase / DBoW3::Database::queryL1 without the
// inverted file: one launch gives the common-word count and the L1 score of every query against every stored row.
//
//   store          one pool of 8-byte units.  Row e = [weight: n doubles][word: n int32, padded to a unit] at rows[e].x units; the row table
//                  {offset in units, n or -1 for a dead row} lives on the host and travels with every query (8 bytes per row), so add is ONE
//                  upload (the row) and erase / clear touch no device memory.  The pool grows geometrically with a device-to-device copy.
//   k_kfdb_query   grid (blocks of entries, query); the workgroup stages the query's words in LDS (32 KiB for YGZ_KFDB_MAX_WORDS), each of its
//                  four wavefronts then walks entries.  A wavefront reads its row 64 words at a time, coalesced; every lane finds its word in
//                  the query by a branch-free lower bound (at most 14 LDS reads, the same count in every lane); a lane that hit fetches the
//                  two weights and forms its term fabs(v - w) - fabs(v) - fabs(w); __ballot gives the hits, their popcount the common words,
//                  and the wavefront adds the terms of the set bits lowest lane first, carried across the chunks: the sum order of
//                  DBoW3::L1Scoring::score (ascending shared words, one addition after the other).  No atomics, no wait for another workgroup.
//
// The arithmetic is that of tests/kfdb_ref.c, bit for bit.  Every index the kernel forms comes from the row table the library wrote itself and
// from the query offsets the entry point validated: the lower bound reads s_word[t - 1] with 1 <= t <= n_q only.
#include "ygz_internal.h"
#include <cmath>
#include <new>
#include <string.h>

#define KFDB_LANES         256
#define KFDB_WAVES         (KFDB_LANES / 64)
#define KFDB_INITIAL_UNITS 65536          // the pool's first allocation: 512 KiB
#define KFDB_BLOCKS        2048           // workgroups a launch aims at

struct ygz_kfdb {
    ygz_hip_ctx *ctx = nullptr;
    double *pool = nullptr;               // device
    size_t cap = 0, used = 0;             // 8-byte units
    std::vector<int2> rows;               // {offset in units, words; -1: dead}
    std::vector<int32_t> words;           // words of every row since the last clear, dead rows included
    int n_alive = 0;
};

namespace {

__device__ __forceinline__ double kfdb_readlane_d(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(KFDB_LANES) void k_kfdb_query(int n_entries, const int2 *__restrict__ rows, const double *__restrict__ pool,
                                                           const int32_t *__restrict__ q_off, const int32_t *__restrict__ q_word,
                                                           const double *__restrict__ q_weight, int32_t *__restrict__ common,
                                                           double *__restrict__ score)
{
    const int q = (int)blockIdx.y;
    const int qa = q_off[q], qn = q_off[q + 1] - qa;
#ifdef YGZ_KFDB_QUERY_THROUGH_L2
    const int32_t *s_word = q_word + qa;                                         // A/B only: the search reads the query through L2
#else
    __shared__ int32_t s_word[YGZ_KFDB_MAX_WORDS];
    for (int i = (int)threadIdx.x; i < qn; i += KFDB_LANES) s_word[i] = q_word[qa + i];
    __syncthreads();
#endif
    const int lane = ygz_lane();
    const int top = qn > 0 ? 1 << (31 - __clz(qn)) : 0;                          // the largest power of two <= qn
    for (int e = (int)blockIdx.x * KFDB_WAVES + (int)(threadIdx.x >> 6); e < n_entries; e += (int)gridDim.x * KFDB_WAVES) {
        const int2 r = rows[e];
        const size_t o = (size_t)q * (size_t)n_entries + (size_t)e;
        if (r.y < 0) {
            if (lane == 0) { common[o] = -1; score[o] = 0.0; }
            continue;
        }
        const double *wt = pool + (size_t)r.x;
        const int32_t *wd = reinterpret_cast<const int32_t *>(wt + r.y);
        double s = 0.0;
        int c = 0;
        for (int base = 0; base < r.y; base += 64) {
            const int i = base + lane;
            bool hit = false;
            double t = 0.0;
            if (i < r.y) {
                const int32_t w = wd[i];
                int lo = 0;                                                       // words of the query below w
                for (int step = top; step >= 1; step >>= 1) {
                    const int u = lo + step;
                    if (u <= qn && s_word[u - 1] < w) lo = u;
                }
                if (lo < qn && s_word[lo] == w) {
                    hit = true;
                    const double v = q_weight[qa + lo], x = wt[i];
                    t = fabs(v - x) - fabs(v) - fabs(x);
                }
            }
            unsigned long long m = __ballot(hit);
            c += __popcll(m);
            while (m) {                                                           // wave-uniform: the hits in ascending word order
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                s += kfdb_readlane_d(t, l);
                m &= m - 1;
            }
        }
        if (lane == 0) { common[o] = c; score[o] = -s / 2.0; }
    }
}

size_t row_units(int n) { return (size_t)n + ((size_t)n + 1) / 2; }

// words >= 0 and strictly ascending, weights finite and > 0
bool vector_ok(const int32_t *word, const double *weight, int n)
{
    for (int i = 0; i < n; ++i) {
        if (word[i] < 0 || (i > 0 && word[i] <= word[i - 1])) return false;
        if (!(weight[i] > 0) || !std::isfinite(weight[i])) return false;
    }
    return true;
}

// room for `need` units: the next capacity is at least twice the last; the rows move with one device-to-device copy on the context's stream
int reserve(ygz_kfdb *db, size_t need)
{
    if (need <= db->cap) return YGZ_OK;
    ygz_hip_ctx *ctx = db->ctx;
    size_t cap = db->cap ? 2 * db->cap : (size_t)KFDB_INITIAL_UNITS;
    while (cap < need) cap *= 2;
    double *p = nullptr;
    YGZ_HIPCHK(ctx, hipMalloc(&p, cap * 8));
    if (db->pool) {
        hipError_t e = db->used ? hipMemcpyAsync(p, db->pool, db->used * 8, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipFree(p); ctx->last_hip_error = (int)e; return YGZ_E_HIP; }
        (void)hipFree(db->pool);
    }
    db->pool = p; db->cap = cap;
    return YGZ_OK;
}

}  // namespace

extern "C" {

int ygz_hip_kfdb_create(ygz_hip_ctx *ctx, ygz_kfdb **db)
{
    if (!db) return YGZ_E_INVALID;
    *db = nullptr;
    if (!ctx) return YGZ_E_INVALID;
    ygz_kfdb *d = new (std::nothrow) ygz_kfdb;
    if (!d) return YGZ_E_HIP;
    d->ctx = ctx;                                   // device memory is allocated by the first add
    *db = d;
    return YGZ_OK;
}

void ygz_hip_kfdb_destroy(ygz_kfdb *db)
{
    if (!db) return;
    if (db->pool) {
        YgzDeviceGuard dg_((const ygz_hip_ctx *)db->ctx);
        (void)hipStreamSynchronize(db->ctx->stream);
        (void)hipFree(db->pool);
    }
    delete db;
}

int ygz_hip_kfdb_add(ygz_kfdb *db, const int32_t *word, const double *weight, int n, int32_t *entry)
{
    if (!entry || (n != 0 && (!word || !weight))) return YGZ_E_INVALID;
    if (n > YGZ_KFDB_MAX_WORDS || (db && db->rows.size() >= (size_t)YGZ_KFDB_MAX_ENTRIES)) return YGZ_E_CAPACITY;
    if (n < 0 || !vector_ok(word, weight, n)) return YGZ_E_INVALID;
    if (!db) return YGZ_E_INVALID;
    ygz_hip_ctx *ctx = db->ctx;
    const size_t units = row_units(n);
    if (n > 0) {
        YgzDeviceGuard dg_(ctx);
        const int rc = reserve(db, db->used + units);
        if (rc != YGZ_OK) return rc;
        uint8_t *up = (uint8_t *)ygz_stage(ctx, units * 8);
        if (!up) return YGZ_E_HIP;
        memcpy(up, weight, (size_t)n * 8);
        memcpy(up + (size_t)n * 8, word, (size_t)n * 4);
        if (n & 1) memset(up + (size_t)n * 12, 0, 4);
        YGZ_HIPCHK(ctx, hipMemcpyAsync(db->pool + db->used, up, units * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    *entry = (int32_t)db->rows.size();
    db->rows.push_back(make_int2((int)db->used, n));
    db->words.push_back(n);
    db->used += units;
    ++db->n_alive;
    return YGZ_OK;
}

int ygz_hip_kfdb_erase(ygz_kfdb *db, int32_t entry)
{
    if (!db || entry < 0 || (size_t)entry >= db->rows.size()) return YGZ_E_INVALID;
    if (db->rows[entry].y >= 0) { db->rows[entry].y = -1; --db->n_alive; }
    return YGZ_OK;
}

int ygz_hip_kfdb_clear(ygz_kfdb *db)
{
    if (!db) return YGZ_E_INVALID;
    // uploads of earlier adds still in flight write below `used`: in stream order before anything a later add sends there
    db->rows.clear(); db->words.clear();
    db->used = 0; db->n_alive = 0;
    return YGZ_OK;
}

int ygz_hip_kfdb_info(const ygz_kfdb *db, int32_t *n_entries, int32_t *n_alive, int64_t *n_words)
{
    if (!db) return YGZ_E_INVALID;
    if (n_entries) *n_entries = (int32_t)db->rows.size();
    if (n_alive) *n_alive = db->n_alive;
    if (n_words) {
        int64_t s = 0;
        for (int32_t w : db->words) s += w;
        *n_words = s;
    }
    return YGZ_OK;
}

int ygz_hip_kfdb_query(ygz_kfdb *db, int n_queries, const int32_t *q_offsets, const int32_t *q_word, const double *q_weight, int32_t *common,
                       double *score)
{
    if (!q_offsets || !q_word || !q_weight || !common || !score) return YGZ_E_INVALID;
    if (n_queries > YGZ_KFDB_MAX_QUERIES) return YGZ_E_CAPACITY;
    for (int q = 0; q < n_queries; ++q)
        if ((long long)q_offsets[q + 1] - (long long)q_offsets[q] > (long long)YGZ_KFDB_MAX_WORDS) return YGZ_E_CAPACITY;
    if (n_queries < 1 || q_offsets[0] != 0) return YGZ_E_INVALID;
    for (int q = 0; q < n_queries; ++q)
        if (q_offsets[q + 1] < q_offsets[q]) return YGZ_E_INVALID;
    for (int q = 0; q < n_queries; ++q)
        if (!vector_ok(q_word + q_offsets[q], q_weight + q_offsets[q], q_offsets[q + 1] - q_offsets[q])) return YGZ_E_INVALID;
    if (!db || db->rows.empty()) return YGZ_E_INVALID;
    ygz_hip_ctx *ctx = db->ctx;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const size_t Q = (size_t)n_queries, W = (size_t)q_offsets[n_queries], E = db->rows.size();
    // [offsets | rows | weights | words) goes up, [score | common) comes back
    YgzBlobLayout L;
    const size_t o_off = L.add_n<int32_t>(Q + 1), o_rows = L.add_n<int2>(E), o_wt = L.add_n<double>(W), o_wd = L.add_n<int32_t>(W), in_end = L.end;
    const size_t o_score = L.add_n<double>(Q * E), o_common = L.add_n<int32_t>(Q * E), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_KFDB, total, total, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_off, q_offsets, (Q + 1) * 4);
    memcpy(b.host + o_rows, db->rows.data(), E * 8);
    memcpy(b.host + o_wt, q_weight, W * 8);
    memcpy(b.host + o_wd, q_word, W * 4);
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    const int per_query = KFDB_BLOCKS / n_queries > 1 ? KFDB_BLOCKS / n_queries : 1;
    const int need = ygz_div_up((int)E, KFDB_WAVES);
    const dim3 grid((unsigned)(need < per_query ? need : per_query), (unsigned)n_queries);
    // a database whose rows are all empty has no pool: the kernel then reads no row
    YGZ_LAUNCH(ctx, KID_COUNT, k_kfdb_query, grid, dim3(KFDB_LANES), (int)E, ygz_at<const int2>(b.dev, o_rows), (const double *)db->pool,
               ygz_at<const int32_t>(b.dev, o_off), ygz_at<const int32_t>(b.dev, o_wd), ygz_at<const double>(b.dev, o_wt),
               ygz_at<int32_t>(b.dev, o_common), ygz_at<double>(b.dev, o_score));
    if ((rc = ygz_blob_fetch(ctx, b, o_score, total)) != YGZ_OK) return rc;
    memcpy(score, b.host + o_score, Q * E * 8);
    memcpy(common, b.host + o_common, Q * E * 4);
    return YGZ_OK;
}

}  // extern "C"
