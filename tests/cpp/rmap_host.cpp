// The host-only logic of the resident map (ygz_slam_amd/csrc/rmap_host.h) under the sanitizers, without a device: a stand-alone program with its
// own main.  Every array it hands over has exactly its size, so a read or a write past one is seen.
//   rmap_host rows     ygz_rmap_rows_ok against a brute-force test (range, duplicates) on crafted and random index lists; the `seen` table is
//                      left all zero whatever the answer
//   rmap_host delta    ygz_rmap_check_delta: every refusal once, and accepted deltas
//   rmap_host arrays   ygz_rmap_check_arrays on a small valid map and on that map with one field broken at a time, in the header's order
//   rmap_host layout   the three layouts: arrays do not overlap, lie at multiples of 256, end inside the block, and overflow is reported
// Each mode prints "<mode> ok <cases>" and exits 0, or prints what failed and exits 1; without an argument it prints its usage and exits 2.
#include "../../ygz_slam_amd/csrc/rmap_host.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

namespace {

int fail(const char *what, long a = 0, long b = 0)
{
    printf("FAILED %s %ld %ld\n", what, a, b);
    return 1;
}

bool brute_rows(int n, const int32_t *idx, int limit)
{
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= limit) return false;
        for (int j = 0; j < i; ++j)
            if (idx[j] == idx[i]) return false;
    }
    return true;
}

int rows()
{
    std::mt19937 rng(7);
    std::vector<uint8_t> seen;
    int cases = 0;
    const auto one = [&](const std::vector<int32_t> &v, int limit) {
        std::unique_ptr<int32_t[]> exact(new int32_t[v.size() ? v.size() : 1]);       // exactly its size
        std::copy(v.begin(), v.end(), exact.get());
        const bool got = ygz_rmap_rows_ok((int)v.size(), v.empty() ? nullptr : exact.get(), limit, seen);
        ++cases;
        if (got != brute_rows((int)v.size(), exact.get(), limit)) return false;
        return std::all_of(seen.begin(), seen.end(), [](uint8_t s) { return s == 0; });
    };
    if (!one({}, 5) || !one({ 0 }, 1) || !one({ 1 }, 1) || !one({ -1 }, 4) || !one({ 3, 2, 1, 0 }, 4) || !one({ 3, 2, 1, 3 }, 4) ||
        !one({ 0, 0 }, 4) || !one({ 2, 4 }, 4) || !one({ 0, 1, 2, 3, -5 }, 4) || !one({ 5 }, 0))
        return fail("crafted rows", cases);
    std::vector<uint8_t> none;
    int32_t some[1] = { 0 };
    if (ygz_rmap_rows_ok(-1, some, 4, none) || ygz_rmap_rows_ok(1, nullptr, 4, none)) return fail("a negative count or a null array");
    for (int t = 0; t < 400; ++t) {
        const int limit = 1 + (int)(rng() % 300), n = (int)(rng() % 40);
        std::vector<int32_t> v((size_t)n);
        for (int32_t &x : v) x = (int32_t)(rng() % (unsigned)(limit + (t % 5 == 0 ? 2 : 0))) - (t % 7 == 0 ? 1 : 0);
        if (!one(v, limit)) return fail("random rows", t);
    }
    // a permutation of a large map is accepted, and refused once one entry repeats
    std::vector<int32_t> perm(100000);
    for (size_t i = 0; i < perm.size(); ++i) perm[i] = (int32_t)i;
    std::shuffle(perm.begin(), perm.end(), rng);
    if (!ygz_rmap_rows_ok((int)perm.size(), perm.data(), (int)perm.size(), seen)) return fail("permutation");
    perm[99999] = perm[5];
    if (ygz_rmap_rows_ok((int)perm.size(), perm.data(), (int)perm.size(), seen)) return fail("repeated entry");
    if (!std::all_of(seen.begin(), seen.end(), [](uint8_t s) { return s == 0; })) return fail("seen left dirty");
    printf("rows ok %d\n", cases + 2);
    return 0;
}

int delta()
{
    const int INV = YGZ_E_INVALID, P = 10, K = 4, Kc = 3;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t pi[3] = { 9, 0, 4 }, pi_out[3] = { 9, 10, 4 }, pi_dup[3] = { 4, 0, 4 }, ki[2] = { 3, 0 }, ki_out[2] = { 4, 0 }, ki_dup[2] = { 2, 2 };
    const int32_t ci[2] = { 2, 1 }, ci_out[2] = { -1, 1 }, ci_dup[2] = { 1, 1 };
    const double pw[9] = { 1, 2, 3, 4, 5, 6, 7, 8, 9 }, pw_nan[9] = { 1, 2, 3, 4, nan, 6, 7, 8, 9 }, c[6] = { 0, 0, 0, 1, 1, 1 }, c_inf[6] = { 0, 0, 0, 1, inf, 1 };
    const uint8_t kb[2] = { 1, 0 };
    int cases = 0;
    const auto is = [&](int rc, int want) { ++cases; return rc == want; };
    if (!is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki, kb, 2, ci, c), YGZ_OK) || !is(ygz_rmap_check_delta(P, K, Kc, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr), YGZ_OK) ||
        !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr), YGZ_OK))
        return fail("accepted deltas", cases);
    if (!is(ygz_rmap_check_delta(P, K, Kc, 3, pi_out, pw, 2, ki, kb, 2, ci, c), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 3, pi_dup, pw, 2, ki, kb, 2, ci, c), INV) ||
        !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki_out, kb, 2, ci, c), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki_dup, kb, 2, ci, c), INV) ||
        !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki, kb, 2, ci_out, c), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki, kb, 2, ci_dup, c), INV) ||
        !is(ygz_rmap_check_delta(P, K, Kc, -1, pi, pw, 0, nullptr, nullptr, 0, nullptr, nullptr), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 3, nullptr, pw, 0, nullptr, nullptr, 0, nullptr, nullptr), INV) ||
        !is(ygz_rmap_check_delta(P, K, Kc, 0, nullptr, nullptr, 2, ki, nullptr, 0, nullptr, nullptr), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 0, nullptr, nullptr, 0, nullptr, nullptr, 2, ci, nullptr), INV) ||
        !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw_nan, 2, ki, kb, 2, ci, c), INV) || !is(ygz_rmap_check_delta(P, K, Kc, 3, pi, pw, 2, ki, kb, 2, ci, c_inf), INV))
        return fail("refused deltas", cases);
    printf("delta ok %d\n", cases);
    return 0;
}

struct Small {
    // two keyframes, three points, two centres
    uint8_t kf_bad[2] = { 0, 0 }, pt_bad[3] = { 0, 1, 0 }, desc[96] = { 0 }, has[3] = { 1, 1, 0 };
    int32_t cov[2] = { 1, -1 }, off[4] = { 0, 2, 2, 3 }, kf[3] = { 0, 1, 1 }, feat[3] = { 5, 0, 7 };
    double centre[6] = { 0, 0, 0, 1, 0, 0 }, pw[9] = { 0, 0, 4, 1, 0, 4, 2, 0, 4 };
    int32_t a_off[4] = { 0, 1, 3, 3 }, a_kf[3] = { 1, 0, 0 }, a_lv[3] = { 0, 30, -2 };
    ygz_map_arrays m;
    Small()
    {
        memset(&m, 0, sizeof m);
        m.n_keyframes = 2; m.n_cov = 1; m.n_points = 3; m.n_centres = 2;
        m.kf_bad = kf_bad; m.cov = cov; m.offsets = off; m.kf = kf; m.feat = feat; m.pt_bad = pt_bad;
        m.centre = centre; m.a_offsets = a_off; m.a_kf = a_kf; m.a_level = a_lv; m.pw = pw; m.pt_desc = desc; m.pt_has_desc = has;
    }
    int check() { int n_obs = -5, n_rows = -5; const int rc = ygz_rmap_check_arrays(&m, &n_obs, &n_rows); return rc == YGZ_OK ? (n_obs == 3 && n_rows == 3 ? 0 : -1000) : (n_obs == -5 && n_rows == -5 ? rc : -1000); }
};

int arrays()
{
    const int INV = YGZ_E_INVALID, CAP = YGZ_E_CAPACITY;
    int cases = 0, n_obs = 0, n_rows = 0;
    const auto is = [&](int rc, int want) { ++cases; return rc == want; };
    Small ok;
    if (!is(ok.check(), 0) || !is(ygz_rmap_check_arrays(nullptr, &n_obs, &n_rows), INV)) return fail("the valid map", cases);
    { Small s; s.m.pt_bad = nullptr; s.m.pt_has_desc = nullptr; if (!is(s.check(), 0)) return fail("optional arrays"); }
    // the selection side
    { Small a; a.m.kf_bad = nullptr; Small b; b.m.offsets = nullptr; Small c; c.m.kf = nullptr; Small d; d.m.feat = nullptr; Small e; e.m.cov = nullptr;
      Small f; f.m.n_keyframes = 0; Small g; g.m.n_cov = -1; Small h; h.m.n_points = 0;
      if (!is(a.check(), INV) || !is(b.check(), INV) || !is(c.check(), INV) || !is(d.check(), INV) || !is(e.check(), INV) || !is(f.check(), INV) || !is(g.check(), INV) || !is(h.check(), INV))
          return fail("selection nulls and counts", cases); }
    { Small a; a.m.n_keyframes = YGZ_LMS_MAX_KEYFRAMES + 1; a.off[0] = 1; Small b; b.m.n_cov = YGZ_LMS_MAX_COV + 1; b.off[0] = 1;
      if (!is(a.check(), CAP) || !is(b.check(), CAP)) return fail("selection capacities before the offsets", cases); }
    { Small a; a.off[0] = 1; Small b; b.off[2] = 1; Small c; c.kf[1] = 2; Small d; d.kf[0] = 1; Small e; e.feat[2] = YGZ_LMS_MAX_FEATURES; Small f; f.feat[0] = -1;
      Small g; g.cov[0] = 2; Small h; h.cov[1] = -2;
      if (!is(a.check(), INV) || !is(b.check(), INV) || !is(c.check(), INV) || !is(d.check(), INV) || !is(e.check(), INV) || !is(f.check(), INV) || !is(g.check(), INV) || !is(h.check(), INV))
          return fail("selection offsets, observations, cov", cases); }
    // the attribute side
    { Small a; a.m.centre = nullptr; Small b; b.m.pw = nullptr; Small c; c.m.a_offsets = nullptr; Small d; d.m.a_kf = nullptr; Small e; e.m.a_level = nullptr; Small f; f.m.n_centres = 0;
      Small g; g.m.n_centres = YGZ_MAP_MAX_KEYFRAMES + 1; g.a_off[0] = 1;
      if (!is(a.check(), INV) || !is(b.check(), INV) || !is(c.check(), INV) || !is(d.check(), INV) || !is(e.check(), INV) || !is(f.check(), INV) || !is(g.check(), CAP))
          return fail("attribute nulls, counts, capacity", cases); }
    { Small a; a.a_off[0] = 1; Small b; b.a_off[3] = 2; Small c; c.a_kf[0] = 2; Small d; d.a_kf[2] = -1; Small e; e.a_lv[0] = 31;
      Small f; f.centre[4] = std::numeric_limits<double>::infinity(); Small g; g.pw[8] = std::numeric_limits<double>::quiet_NaN(); Small h; h.m.pt_desc = nullptr;
      if (!is(a.check(), INV) || !is(b.check(), INV) || !is(c.check(), INV) || !is(d.check(), INV) || !is(e.check(), INV) || !is(f.check(), INV) || !is(g.check(), INV) || !is(h.check(), INV))
          return fail("attribute offsets, rows, finiteness, descriptor", cases); }
    // a point with too many observations is a capacity, found before the observations are read
    {
        std::vector<int32_t> off = { 0, YGZ_MAP_MAX_OBS_PER_POINT + 1, YGZ_MAP_MAX_OBS_PER_POINT + 1, YGZ_MAP_MAX_OBS_PER_POINT + 1 };
        Small a; a.m.offsets = off.data();
        if (!is(a.check(), CAP)) return fail("observations per point");
    }
    printf("arrays ok %d\n", cases);
    return 0;
}

bool spans_ok(std::vector<std::pair<size_t, size_t>> s, size_t end)
{
    std::sort(s.begin(), s.end());
    size_t at = 0;
    for (const auto &p : s) {
        if (p.first % 256 || p.first < at) return false;
        at = p.first + p.second;
    }
    return at <= end && end % 256 == 0;
}

int layout()
{
    std::mt19937 rng(11);
    int cases = 0;
    for (int t = 0; t < 300; ++t, ++cases) {
        const size_t K = 1 + rng() % 50, C = rng() % 5, P = 1 + rng() % 3000, N = rng() % 9000, Kc = 1 + rng() % 60, R = rng() % 9000;
        const RmapStore S(K, C, P, N, Kc, R);
        if (S.bad || !spans_ok({ { S.o_kbad, K }, { S.o_pbad, P }, { S.o_has, P }, { S.o_cov, 4 * K * C }, { S.o_off, 4 * (P + 1) }, { S.o_obs, 4 * N }, { S.o_koff, 4 * (K + 1) },
                                 { S.o_kpt, 4 * N }, { S.o_centre, 24 * Kc }, { S.o_pw, 24 * P }, { S.o_aoff, 4 * (P + 1) }, { S.o_akf, 4 * R }, { S.o_alv, 4 * R },
                                 { S.o_desc, 32 * P }, { S.o_dmax, 8 * P }, { S.o_nrm, 24 * P }, { S.o_state, 4 * P } }, S.end) || S.in_end > S.o_dmax || S.o_desc + 32 * P > S.in_end)
            return fail("store layout", t);
        const size_t F = 1 + rng() % 20, E = rng() % 5000, MP = 1 + rng() % 700, cells = 1 + rng() % 800;
        const RmapCall L(F, K, E, MP, cells);
        if (L.bad || !spans_ok({ { L.o_foff, 4 * (F + 1) }, { L.o_fpt, 4 * E }, { L.o_ref, 4 * F }, { L.o_nvot, 4 * F }, { L.o_nloc, 4 * F }, { L.o_npt, 4 * F }, { L.o_ncut, 4 * F },
                                 { L.o_nrem, 4 * F }, { L.o_lkf, 4 * F * K }, { L.o_lpt, 4 * F * MP }, { L.o_prior, 4 * F * cells }, { L.o_votes, 4 * F * K }, { L.o_npt0, 4 * F },
                                 { L.o_lpt0, 4 * F * MP }, { L.o_fprior, 4 * E }, { L.o_rank, 2 * F * K }, { L.o_cnt, 4 * F * K }, { L.o_start, 4 * F * (K + 1) },
                                 { L.o_lft, 4 * F * MP }, { L.o_moved, 4 * F * MP } }, L.end))
            return fail("call layout", t);
        if (L.back_end(true, false) != L.out_end || L.back_end(false, true) != L.prior_end || L.back_end(false, false) != L.small_end ||
            !(L.in_end <= L.o_ref && L.small_end <= L.prior_end && L.prior_end <= L.out_end && L.out_end <= L.end && L.o_lpt + 4 * F * MP <= L.small_end))
            return fail("call copy-back ranges", t);
        const size_t np = rng() % 400, nk = rng() % 9, nc = rng() % 9;
        const bool a = rng() & 1, b = rng() & 1, c = rng() & 1, d = rng() & 1;
        const RmapDelta D(np, a, b, c, d, nk, nc);
        if (D.bad || !spans_ok({ { D.o_pidx, 4 * np }, { D.o_pw, a ? 24 * np : 0 }, { D.o_desc, b ? 32 * np : 0 }, { D.o_pbad, c ? np : 0 }, { D.o_has, d ? np : 0 },
                                 { D.o_kidx, 4 * nk }, { D.o_kbad, nk }, { D.o_cidx, 4 * nc }, { D.o_centre, 24 * nc } }, D.end))
            return fail("delta layout", t);
    }
    const size_t huge = std::numeric_limits<size_t>::max() / 16;
    if (!RmapStore(4, 2, huge, 10, 3, 10).bad || !RmapCall(huge, 4, 10, 16, 10).bad || !RmapDelta(huge, true, true, true, true, 1, 1).bad) return fail("overflow is reported");
    if (ygz_rmap_grown(1000) != 1506 || ygz_rmap_grown(0) != 256) return fail("growth rule");
    printf("layout ok %d\n", cases + 2);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "rows") == 0) return rows();
    if (argc == 2 && strcmp(argv[1], "delta") == 0) return delta();
    if (argc == 2 && strcmp(argv[1], "arrays") == 0) return arrays();
    if (argc == 2 && strcmp(argv[1], "layout") == 0) return layout();
    fprintf(stderr, "usage: rmap_host rows | delta | arrays | layout\n");
    return 2;
}
