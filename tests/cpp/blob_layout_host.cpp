// YgzBlobLayout (ygz_slam_amd/csrc/ygz_blob.h) on the host, without a device and without a HIP header.  Built with
// -fsanitize=address,undefined and run as a program by tests/test_blob_layout_host.py.  It checks the helper, not the entry points: the
// PnP, culling and database blocks below are RESTATED here (a .hip file cannot be included), so a swapped add in pnp.hip, cull.hip or
// kfdb.hip shows in the GPU suites, not in this program.
#include "ygz_blob.h"

#include <cstdio>
#include <initializer_list>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

// the recurrence every entry point used to write out by hand: x = o; o = al(o + bytes)
static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// the total of a block by plain arithmetic, without the recurrence: every array takes whole units of 256 bytes
static size_t total_of(std::initializer_list<size_t> bytes)
{
    size_t units = 0;
    for (size_t b : bytes) units += b / 256 + (b % 256 != 0);
    return units * 256;
}

static void ladder(const std::vector<size_t> &sizes)
{
    YgzBlobLayout L;
    size_t o = 0;
    for (size_t n : sizes) {
        const size_t before = L.end, at = L.add(n);
        CHECK(at == o && at == before);
        o = al(o + n);
        CHECK(L.end == o && L.end % 256 == 0 && at % 256 == 0 && !L.bad());
        if (n == 0) CHECK(L.end == before);
    }
}

// the three blocks restated after pnp.hip layout(), cull.hip ygz_hip_cull_keyframes / ygz_hip_keyframe_redundancy and kfdb.hip
// ygz_hip_kfdb_query, with the sizes of their structures as numbers: PnpIn 56 bytes, ygz_pnp_result 176 (a static_assert in pnp.hip holds
// both), a row of the table 8 (int2)
struct Pnp176 { unsigned char b[176]; };
struct Row8 { unsigned char b[8]; };

static size_t pnp_total(size_t P, size_t N, size_t it)
{
    YgzBlobLayout B;
    const size_t H = P * it;
    B.add(56); B.add_n<int32_t>(P + 1); B.add_n<double>(N * 3); B.add_n<double>(N * 2); B.add_n<int32_t>(H * 3);
    B.add_n<Pnp176>(P); B.add(N);
    B.add_n<int32_t>(H); B.add_n<int32_t>(H * 4); B.add_n<double>(H * 4 * 12);
    CHECK(!B.bad());
    return B.end;
}
static size_t cull_walk_total(size_t P, size_t N, size_t C, size_t M)
{
    YgzBlobLayout L;
    L.add_n<int32_t>(P + 1); L.add_n<int32_t>(N); L.add_n<int32_t>(C); L.add_n<int32_t>(C + 1); L.add_n<int32_t>(M + 1); L.add_n<int32_t>(M + 1);
    L.add_n<int32_t>(P); L.add_n<int32_t>(3 * C); L.add(P);
    CHECK(!L.bad());
    return L.end;
}
static size_t cull_counts_total(size_t P, size_t N, size_t K)
{
    YgzBlobLayout L;
    L.add_n<int32_t>(P + 1); L.add_n<int32_t>(N); L.add_n<int32_t>(N); L.add_n<int32_t>(2 * K);
    CHECK(!L.bad());
    return L.end;
}
static size_t kfdb_total(size_t Q, size_t E, size_t W)
{
    YgzBlobLayout L;
    L.add_n<int32_t>(Q + 1); L.add_n<Row8>(E); L.add_n<double>(W); L.add_n<int32_t>(W); L.add_n<double>(Q * E); L.add_n<int32_t>(Q * E);
    CHECK(!L.bad());
    return L.end;
}

int main()
{
    for (size_t n : { 0, 1, 255, 256, 257 }) ladder({ n });
    for (size_t n : { 0, 1, 255, 256, 257 }) ladder({ 1, n, 1 });
    ladder({ 0, 0, 1, 255, 0, 256, 257, 0, 4097, 3, 65536, 0, 1000003, 12, 0 });
    CHECK(ygz_round_up_256(0) == 0 && ygz_round_up_256(1) == 256 && ygz_round_up_256(256) == 256 && ygz_round_up_256(257) == 512);

    {   // add_n is add(count * sizeof(T)); an absent array (count 0) takes no room
        YgzBlobLayout L;
        CHECK(L.add_n<double>(3) == 0 && L.end == 256);
        CHECK(L.add_n<int32_t>(0) == 256 && L.end == 256);
        CHECK(L.add_n<int32_t>(65) == 256 && L.end == 768);
        CHECK(L.add_n<uint8_t>(1) == 768 && L.end == 1024 && !L.bad());
    }
    {   // an overflowing size marks the layout bad for good instead of wrapping
        YgzBlobLayout L;
        L.add(100);
        L.add_n<double>(SIZE_MAX / 4);
        CHECK(L.bad() && L.end == YgzBlobLayout::BAD);
        L.add(1);
        CHECK(L.bad());
        YgzBlobLayout M;
        M.add(SIZE_MAX - 100);                     // the bytes fit, their round-up does not
        CHECK(M.bad());
        YgzBlobLayout K;
        K.add(512);
        K.add(SIZE_MAX - 600);                     // the sum wraps
        CHECK(K.bad());
        YgzBlobLayout G;
        G.add_n<double>(SIZE_MAX / 8 - 64);        // the largest sizes that still fit stay good
        CHECK(!G.bad() && G.end % 256 == 0);
    }

    // PnP: P = 1, N = 4, it = 1, and 64 problems of 3072 points at 1024 iterations
    CHECK(pnp_total(1, 4, 1) == total_of({ 56, 8, 96, 64, 12, 176, 4, 4, 16, 384 }));
    CHECK(pnp_total(1, 4, 1) == 11 * 256);         // ten arrays, the 384 bytes of the solutions take two units
    {
        const size_t P = 64, N = 64 * 3072, H = 64 * 1024;
        CHECK(pnp_total(P, N, 1024) == total_of({ 56, (P + 1) * 4, N * 24, N * 16, H * 12, P * 176, N, H * 4, H * 16, H * 384 }));
    }
    // culling: OK_CASE of tests/test_cull_surface_build.py (2 points, 3 observations, 3 keyframes, candidates 2 and 0 with 2 observations), and
    // 4096 keyframes, all candidates, over 1 048 576 observations of as many points
    CHECK(cull_walk_total(2, 3, 2, 2) == total_of({ 12, 12, 8, 12, 12, 12, 8, 24, 2 }) && cull_walk_total(2, 3, 2, 2) == 9 * 256);
    CHECK(cull_counts_total(2, 3, 3) == 4 * 256);
    {
        const size_t K = 4096, N = 1048576, P = N;
        CHECK(cull_walk_total(P, N, K, N) == total_of({ (P + 1) * 4, N * 4, K * 4, (K + 1) * 4, (N + 1) * 4, (N + 1) * 4, P * 4, 3 * K * 4, P }));
        CHECK(cull_counts_total(P, N, K) == total_of({ (P + 1) * 4, N * 4, N * 4, 2 * K * 4 }));
        CHECK(cull_counts_total(P, N, K) == (4194304 + 256) + 4194304 + 4194304 + 32768);
    }
    // keyframe database: 1 query of 1 word against 1 entry, and 64 queries of 8192 words against 4096 entries
    CHECK(kfdb_total(1, 1, 1) == 6 * 256);
    {
        const size_t Q = 64, E = 4096, W = 64 * 8192;
        CHECK(kfdb_total(Q, E, W) == total_of({ (Q + 1) * 4, E * 8, W * 8, W * 4, Q * E * 8, Q * E * 4 }));
        CHECK(kfdb_total(Q, E, W) == 512 + 32768 + 4194304 + 2097152 + 2097152 + 1048576);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
