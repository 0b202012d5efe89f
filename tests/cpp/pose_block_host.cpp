// The host plumbing of the launchers of k_pose_opt (ygz_slam_amd/csrc/pose_block.h) without a device and without a HIP header.  Built with
// -fsanitize=address,undefined and run as a program by tests/test_pose_block_host.py.  Output buffers are sized exactly, so a copy that
// runs past its array is an AddressSanitizer report.
#include "pose_block.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

// the defaults of ygz_hip_default_pose_opt_params, restated
static ygz_pose_opt_params defaults()
{
    ygz_pose_opt_params p;
    p.baseline = 0.0; p.chi2_mono = 5.991; p.chi2_stereo = 7.815;
    p.rounds = 4; p.iterations = 10; p.max_trials = 10; p.robust_rounds = 3; p.min_edges = 3; p.min_inliers = 10;
    p.min_rel_decrease = 0.0;
    return p;
}

static void params()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(ygz_pose_params_ok(defaults()));
    ygz_pose_opt_params p;
    // every exact limit is accepted, every limit crossed by one is refused
    for (int v : { 1, YGZ_POPT_MAX_ROUNDS }) { p = defaults(); p.rounds = v; CHECK(ygz_pose_params_ok(p)); }
    for (int v : { 0, YGZ_POPT_MAX_ROUNDS + 1 }) { p = defaults(); p.rounds = v; CHECK(!ygz_pose_params_ok(p)); }
    for (int v : { 1, YGZ_POPT_MAX_STEPS }) {
        p = defaults(); p.iterations = v; CHECK(ygz_pose_params_ok(p));
        p = defaults(); p.max_trials = v; CHECK(ygz_pose_params_ok(p));
    }
    for (int v : { 0, YGZ_POPT_MAX_STEPS + 1 }) {
        p = defaults(); p.iterations = v; CHECK(!ygz_pose_params_ok(p));
        p = defaults(); p.max_trials = v; CHECK(!ygz_pose_params_ok(p));
    }
    for (double v : { 0.0, -1.0, nan, inf }) {
        p = defaults(); p.chi2_mono = v; CHECK(!ygz_pose_params_ok(p));
        p = defaults(); p.chi2_stereo = v; CHECK(!ygz_pose_params_ok(p));
    }
    p = defaults(); p.min_rel_decrease = nan; CHECK(!ygz_pose_params_ok(p));
    p = defaults(); p.baseline = nan; CHECK(ygz_pose_params_ok(p));             // the baseline is the caller's to judge
}

static void finite()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(ygz_all_finite(nullptr, 0));
    const std::vector<double> good = { 0.0, -1.5, 1e300, 5e-324, 7.0 };
    CHECK(ygz_all_finite(good.data(), good.size()));
    for (double bad : { nan, inf, -inf })
        for (size_t at : { (size_t)0, good.size() / 2, good.size() - 1 }) {
            std::vector<double> v = good;
            v[at] = bad;
            CHECK(!ygz_all_finite(v.data(), v.size()));
            CHECK(ygz_all_finite(v.data(), at));                                 // the range ends before it
        }
}

// whole units of 256 bytes
static size_t units(size_t bytes) { return (bytes + 255) / 256 * 256; }

static void block(size_t F, size_t cells)
{
    const size_t R8 = F * YGZ_POPT_MAX_ROUNDS, N = F * cells, lead = 3 * 256;
    YgzBlobLayout B;
    B.add(lead - 1);                                                             // something stands in front, as in every entry point
    YgzPoseBlock P;
    P.add_results(B, F);
    const size_t results_end = B.end;
    B.add(1);                                                                    // and between the two groups
    P.add_edges(B, F, cells);
    CHECK(!B.bad());
    const size_t res[7] = { P.inliers, P.rounds_run, P.round_status, P.round_iterations, P.round_cost_initial, P.round_cost_final, P.round_lambda };
    const size_t res_bytes[7] = { F * 4, F * 4, R8 * 4, R8 * 4, R8 * 8, R8 * 8, R8 * 8 };
    const size_t edg[8] = { P.edge_of, P.e_pw, P.e_obs, P.e_level, P.e_kind, P.e_outlier, P.e_chi2, P.edge_end };
    const size_t edg_bytes[8] = { N * 4, N * 24, N * 24, N * 4, N, N, N * 8, F * 4 };
    size_t o = lead;
    for (int k = 0; k < 7; ++k) { CHECK(res[k] == o && res[k] % 256 == 0); if (k) CHECK(res[k] > res[k - 1]); o += units(res_bytes[k]); }
    CHECK(results_end == o);
    o += 256;
    for (int k = 0; k < 8; ++k) { CHECK(edg[k] == o && edg[k] % 256 == 0); if (k) CHECK(edg[k] > edg[k - 1]); o += units(edg_bytes[k]); }
    CHECK(edg[0] > res[6] && B.end == o);
    CHECK(B.end == lead + 2 * units(F * 4) + 2 * units(R8 * 4) + 3 * units(R8 * 8) + 256 + 2 * units(N * 4) + 2 * units(N * 24) + 2 * units(N) +
                       units(N * 8) + units(F * 4));

    // copy_results: seven distinct patterns in the block, outputs of exactly F or F * YGZ_POPT_MAX_ROUNDS elements
    std::vector<uint8_t> up(B.end, 0xEE);
    for (int k = 0; k < 7; ++k)
        for (size_t i = 0; i < res_bytes[k]; ++i) up[res[k] + i] = (uint8_t)(16 * (k + 1) + i % 13);
    std::vector<int32_t> inl(F), run(F), st(R8), it(R8);
    std::vector<double> ci(R8), cf(R8), lam(R8);
    P.copy_results(up.data(), F, inl.data(), run.data(), st.data(), it.data(), ci.data(), cf.data(), lam.data());
    const void *out[7] = { inl.data(), run.data(), st.data(), it.data(), ci.data(), cf.data(), lam.data() };
    for (int k = 0; k < 7; ++k) CHECK(memcmp(out[k], up.data() + res[k], res_bytes[k]) == 0);
    // every output alone, the others absent; then none
    for (int only = 0; only < 7; ++only) {
        std::vector<int32_t> a(only < 2 ? F : R8, -7);
        std::vector<double> d(R8, -7.0);
        P.copy_results(up.data(), F, only == 0 ? a.data() : nullptr, only == 1 ? a.data() : nullptr, only == 2 ? a.data() : nullptr,
                       only == 3 ? a.data() : nullptr, only == 4 ? d.data() : nullptr, only == 5 ? d.data() : nullptr,
                       only == 6 ? d.data() : nullptr);
        CHECK(memcmp(only < 4 ? (const void *)a.data() : (const void *)d.data(), up.data() + res[only], res_bytes[only]) == 0);
        if (only < 4) for (double x : d) CHECK(x == -7.0);
    }
    P.copy_results(up.data(), F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

static void slots()
{
    std::vector<int32_t> list, where(4, -1), place;
    for (int32_t s : { 3, 1, 3, 0, 1 }) place.push_back(ygz_distinct_slot(list, where, s));
    CHECK((list == std::vector<int32_t>{ 3, 1, 0 }));
    CHECK((place == std::vector<int32_t>{ 0, 1, 0, 2, 1 }));
    CHECK((where == std::vector<int32_t>{ 2, 1, -1, 0 }));
}

int main()
{
    params();
    finite();
    for (size_t F : { (size_t)1, (size_t)65 })
        for (size_t cells : { (size_t)1, (size_t)768 }) block(F, cells);
    slots();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
