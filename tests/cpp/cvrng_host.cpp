// The register form of the RANSAC sample sets (ygz_slam_amd/csrc/cvrng_dev.h: ygz_cvrng_words, ygz_cvrng_set3), a stand-alone host program for
// tests/test_cvrng_host.py: built with -fsanitize=address,undefined and linked with tests/pnp_ref.c, it forms the sets the way a lane of
// k_srl_sets does -- from the table of generator words and n alone -- and holds them to pr_sample_sets(n, max_iter), which walks the
// availableIndices array, for every n in 3 .. 4096 and max_iter in { 1, 300, 1024 }.
//   cvrng_host          every n and max_iter; prints the number of sets compared
#include "../../ygz_slam_amd/csrc/cvrng_dev.h"
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" void pr_sample_sets(int n, int max_iter, int32_t *sets);

int main()
{
    const int iters[3] = { 1, 300, 1024 };
    std::vector<uint32_t> words(3 * 1024);
    ygz_cvrng_words(3 * 1024, words.data());
    // the words do not depend on how many are asked for
    std::vector<uint32_t> few(3);
    ygz_cvrng_words(3, few.data());
    if (memcmp(few.data(), words.data(), 12) != 0) { printf("cvrng_host: the first words differ\n"); return 1; }
    long long compared = 0;
    for (int n = 3; n <= 4096; ++n) {
        for (int it : iters) {
            std::vector<int32_t> want(3 * (size_t)it), got(3 * (size_t)it);
            pr_sample_sets(n, it, want.data());
            for (int i = 0; i < it; ++i) ygz_cvrng_set3(words[3 * (size_t)i], words[3 * (size_t)i + 1], words[3 * (size_t)i + 2], n, &got[3 * (size_t)i]);
            for (int i = 0; i < it; ++i) {
                const int32_t *g = &got[3 * (size_t)i], *w = &want[3 * (size_t)i];
                if (g[0] != w[0] || g[1] != w[1] || g[2] != w[2]) {
                    printf("cvrng_host: n %d max_iter %d iteration %d: %d %d %d, pr_sample_sets %d %d %d\n", n, it, i, g[0], g[1], g[2], w[0], w[1], w[2]);
                    return 1;
                }
                if (g[0] == g[1] || g[0] == g[2] || g[1] == g[2] || g[0] < 0 || g[1] < 0 || g[2] < 0 || g[0] >= n || g[1] >= n || g[2] >= n) {
                    printf("cvrng_host: n %d iteration %d: %d %d %d are not three distinct indices\n", n, i, g[0], g[1], g[2]);
                    return 1;
                }
            }
            compared += it;
        }
    }
    printf("cvrng_host: %lld sets equal\n", compared);
    return 0;
}
