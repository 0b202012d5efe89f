// The keyframe-major index of the local-map selection (ygz_slam_amd/csrc/lms_index.h) on the host, without a device: a stand-alone program
// that includes the header the entry point builds its index with, meant to be compiled with -fsanitize=address,undefined.  Each argument is a
// file of int32: n_points, K, offsets [n_points + 1], kf [n_obs], feat [n_obs] (tests/test_lms_index_host.py writes the maps of
// tests/lms_ref.py).  The index is held to a brute-force build: every (keyframe, feature, point) triple, sorted.  Every array has exactly
// its size on the heap, so a write past an end is seen.  Prints "<file name> ok <n_obs>" per file; exit status 1 on a difference.
#include "../../ygz_slam_amd/csrc/lms_index.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>

static bool read_all(const char *path, std::vector<int32_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / 4);
    const bool ok = bytes % 4 == 0 && fread(v.data(), 4, v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: lms_index_host FILE...\n"); return 2; }
    for (int a = 1; a < argc; ++a) {
        std::vector<int32_t> in;
        if (!read_all(argv[a], in) || in.size() < 3) { fprintf(stderr, "%s: unreadable\n", argv[a]); return 2; }
        const int n_points = in[0], K = in[1];
        if (n_points < 1 || K < 1 || in.size() < (size_t)n_points + 3) { fprintf(stderr, "%s: bad header\n", argv[a]); return 2; }
        const std::vector<int32_t> offsets(in.begin() + 2, in.begin() + 3 + n_points);
        const size_t n_obs = (size_t)offsets[(size_t)n_points];
        if (in.size() != (size_t)n_points + 3 + 2 * n_obs) { fprintf(stderr, "%s: bad size\n", argv[a]); return 2; }
        const std::vector<int32_t> kf(in.begin() + 3 + n_points, in.begin() + 3 + n_points + (long)n_obs);
        const std::vector<int32_t> feat(in.begin() + 3 + n_points + (long)n_obs, in.end());
        std::vector<int32_t> koff((size_t)K + 1, -5), kpt(n_obs, -5), kft(n_obs, -5), kpt_only(n_obs, -5);
        ygz_lms_build_index(n_points, offsets.data(), kf.data(), feat.data(), K, koff.data(), kpt.data(), kft.data());
        // brute force: all triples, sorted
        std::vector<std::tuple<int32_t, int32_t, int32_t>> all;
        for (int p = 0; p < n_points; ++p)
            for (int g = offsets[(size_t)p]; g < offsets[(size_t)p + 1]; ++g) all.emplace_back(kf[(size_t)g], feat[(size_t)g], p);
        std::sort(all.begin(), all.end());
        bool ok = koff[0] == 0 && (size_t)koff[(size_t)K] == n_obs;
        for (int k = 0; k < K && ok; ++k) {
            ok = koff[(size_t)k + 1] >= koff[(size_t)k];
            for (int m = koff[(size_t)k]; m < koff[(size_t)k + 1] && ok; ++m)
                ok = all[(size_t)m] == std::make_tuple((int32_t)k, kft[(size_t)m], kpt[(size_t)m]);
        }
        // without the feature array the points are the same
        std::vector<int32_t> koff2((size_t)K + 1, -5);
        ygz_lms_build_index(n_points, offsets.data(), kf.data(), feat.data(), K, koff2.data(), kpt_only.data(), nullptr);
        ok = ok && koff2 == koff && kpt_only == kpt;
        const char *name = strrchr(argv[a], '/');
        printf("%s %s %zu\n", name ? name + 1 : argv[a], ok ? "ok" : "DIFFERS", n_obs);
        if (!ok) return 1;
    }
    return 0;
}
