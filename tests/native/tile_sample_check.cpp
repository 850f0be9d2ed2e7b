// slimm_amd/csrc/tile_plan.h, the sampled count: the capacity rule, the plan's choice of S and the bucket allocation walked
// at their edges.  Stand-alone (g++, -fsanitize=address,undefined); built and run by tests/test_tile_sample_plan.py.  The
// expectations are written out in numbers, not taken from the header's constants.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../slimm_amd/csrc/tile_plan.h"

using namespace slimm;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) {                                                   \
            ++g_failed;                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);           \
        }                                                                \
    } while (0)

static TileLayout layout(uint32_t ntiles, uint32_t ntiles2) {
    TileLayout l;
    l.tile_shift = 14;
    l.ntiles = ntiles;
    l.ntiles2 = ntiles2;
    return l;
}
static TilePlan plan(uint32_t ntiles2, const TileForces& f = TileForces()) {
    return tile_plan(ntiles2, f, static_cast<uint64_t>(ntiles2) * 4 <= 144u * 1024u);
}

static void roots() {
    CHECK(tile_isqrt_up(0) == 0 && tile_isqrt_up(1) == 1 && tile_isqrt_up(2) == 2 && tile_isqrt_up(4) == 2 && tile_isqrt_up(5) == 3);
    CHECK(tile_isqrt_up32(0) == 0 && tile_isqrt_up32(1) == 1 && tile_isqrt_up32(2) == 2 && tile_isqrt_up32(4) == 2 && tile_isqrt_up32(5) == 3);
    CHECK(tile_isqrt_up32(46340u * 46340u) == 46340 && tile_isqrt_up32(46340u * 46340u + 1) == 46341 && tile_isqrt_up32(0x7fffffffu) == 46341);
    for (uint64_t r : {3ull, 1000ull, 65535ull, 65536ull, 94906267ull, 1073741824ull, 2147483647ull}) {  // (r * r < 2^62)
        CHECK(tile_isqrt_up(r * r) == r);        // exact at a square,
        CHECK(tile_isqrt_up(r * r + 1) == r + 1);  // up behind it,
        CHECK(tile_isqrt_up(r * r - 1) == r);    // and up to it from below
    }
}

static void capacities() {
    // cap(c) = S c + S k^2 / 2 + k S ceil(sqrt(4 c + k^2)) / 2 + S.  c = 0: S k^2 + S
    CHECK(tile_cap(0, 2, 8) == 130 && tile_cap(0, 16, 8) == 1040 && tile_cap(0, 4, 8) == 260 && tile_cap(0, 16, 0) == 16);
    CHECK(tile_cap(0, 2, 2) == 10 && tile_cap(0, 4, 2) == 20);
    // S = 2, c = 50: 100 + 64 + 8 * ceil(sqrt(264)) + 2
    CHECK(tile_cap(50, 2, 8) == 100 + 64 + 8 * 17 + 2);
    // the headline: 15 800 entries per stretch, S = 16, c = 988: 15 808 + 512 + 64 * ceil(sqrt(4016)) + 16 = 20 432 (29 %)
    CHECK(tile_cap(988, 16, 8) == 15808 + 512 + 64 * 64 + 16);
    // k = 0: the estimate and the constant
    CHECK(tile_cap(1000, 16, 0) == 16016);
    // the k deviations hold at the TRUE fill: n = cap(c) lies within k sqrt(S n) of S c, n + S + 1 does not lie far outside
    for (uint32_t S : {2u, 4u, 16u})
        for (uint32_t c : {0u, 1u, 2u, 9u, 100u, 988u, 100000u}) {
            const double n = tile_cap(c, S, 8) - S, dev = (n - double(S) * c) / __builtin_sqrt(S * n);
            CHECK(dev >= 8.0 && dev < 8.0 + 1.0);
        }
    // monotone in c, and never below the estimate
    uint32_t before = 0;
    for (uint32_t c = 0; c < 100000; c += 37) {
        const uint32_t cap = tile_cap(c, 16, 8);
        CHECK(cap >= before && cap >= 16u * c + 16u);
        before = cap;
    }
    // counts from 2^28 on (and so near 2^31): saturated, not wrapped; below, the largest that fits is exact
    CHECK(tile_cap(0x7fffffffu, 16, 8) == 0xffffffffu && tile_cap(0x80000000u, 2, 8) == 0xffffffffu);
    CHECK(tile_cap(0xffffffffu, 16, 64) == 0xffffffffu && tile_cap(1u << 28, 2, 0) == 0xffffffffu);
    CHECK(tile_cap((1u << 28) - 1u, 16, 0) == 0xffffffffu);   // 2^32: one too many
    CHECK(tile_cap((1u << 28) - 2u, 16, 0) == 0xfffffff0u);   // 2^32 - 32 + 16
    CHECK(tile_cap((1u << 28) - 1u, 2, 0) == (1u << 29));
    CHECK(tile_cap(0x0fffffffu, 2, 8) == 2u * 0x0fffffffu + 64u + 8u * 32769u + 2u);  // sqrt(2^30 + 60) rounded up
}

static void strides() {
    // the sizes at which S changes: values / (8 copies * tiles) against 1024 S; one tile, so values / 8
    CHECK(tile_sample_stride(0, 1) == 1 && tile_sample_stride(8 * 2047, 1) == 1 && tile_sample_stride(8 * 2048 - 1, 1) == 1);
    CHECK(tile_sample_stride(8 * 2048, 1) == 2 && tile_sample_stride(8 * 4096 - 1, 1) == 2);
    CHECK(tile_sample_stride(8 * 4096, 1) == 4 && tile_sample_stride(8 * 8192 - 1, 1) == 4);
    CHECK(tile_sample_stride(8 * 8192, 1) == 8 && tile_sample_stride(8 * 16384 - 1, 1) == 8);
    CHECK(tile_sample_stride(8 * 16384, 1) == 16 && tile_sample_stride(1ull << 40, 1) == 16);
    CHECK(tile_sample_stride(1000, 0) == 1);  // (no tiles: nothing divides by zero)
    // the headline: 1 B records over 4 888 tiles take 16 in phase A; 120 M selectors over 4 890 tiles would take 2 by size
    CHECK(tile_sample_stride(1000000000ull, 4888) == 16 && tile_sample_stride(120000000ull, 4890) == 2);
    // which paths sample: the rounds with eight copies, nothing else
    const TilePhase A = TilePhase::A, B = TilePhase::B;
    const uint64_t many = 1ull << 40;
    CHECK(tile_run(layout(4000, 4000), plan(4000), A, many, many).path == TilePath::Fused);
    CHECK(tile_run(layout(4000, 4000), plan(4000), A, many, many).sample == 1);
    CHECK(tile_run(layout(4888, 4890), plan(4890), A, many, many).path == TilePath::OrderedRounds);
    CHECK(tile_run(layout(4888, 4890), plan(4890), A, many, many).sample == 16 && tile_run(layout(4888, 4890), plan(4890), B, many, many).sample == 16);
    CHECK(tile_run(layout(4888, 4890), plan(4890), A, 1000000000ull, 1000000000ull).sample == 16);
    CHECK(tile_run(layout(4888, 4890), plan(4890), B, 120000000ull, 1000000000ull).sample == 1);  // (60 M skipped: not worth it)
    CHECK(tile_run(layout(4888, 4890), plan(4890), B, 1000000ull, 1000000000ull).sample == 1);  // 25 per stretch
    // a sample has to leave 112 M values unread, twice what pays for the fit and the empty launches: config 3's phase A
    // (100 M records, S = 2 by the stretches: 50 M skipped) keeps the full count, 224 M at S = 2 sample (to the value)
    CHECK(tile_sample_stride(100000000ull, 611) == 16 && tile_sample_stride(100000000ull, 4888) == 2);
    CHECK(tile_run(layout(4888, 4890), plan(4890), A, 100000000ull, 100000000ull).sample == 1);
    CHECK(tile_run(layout(9000, 9100), plan(9100), A, 223999998ull, 223999998ull).sample == 1);  // (3 111 per stretch: S = 2)
    CHECK(tile_run(layout(9000, 9100), plan(9100), A, 223999999ull, 223999999ull).sample == 2);  // (odd: 112 000 000 skipped)
    CHECK(tile_run(layout(4200, 4300), plan(4300), A, 59000000ull, 59000000ull).sample == 1);   // 1715 per stretch anyway
    CHECK(tile_run(layout(4200, 4300), plan(4300), A, 300000000ull, 300000000ull).sample == 8);  // 8 928 per stretch
    CHECK(tile_run(layout(8000, 8100), plan(8100), A, many, many).path == TilePath::DirectRounds);
    CHECK(tile_run(layout(8000, 8100), plan(8100), A, many, many).sample == 16);
    CHECK(tile_run(layout(8000, 8100), plan(8100), B, 1000, many).path == TilePath::Matrix);
    CHECK(tile_run(layout(8000, 8100), plan(8100), B, 1000, many).sample == 1);
    CHECK(tile_run(layout(20000, 20100), plan(20100), A, many, many).path == TilePath::TwoLevel);
    CHECK(tile_run(layout(20000, 20100), plan(20100), A, many, many).sample == 1);
    CHECK(tile_run(layout(40000, 40100), plan(40100), A, many, many).path == TilePath::DirectAtomics);
    CHECK(tile_run(layout(40000, 40100), plan(40100), A, many, many).sample == 1);
    TileForces f;
    f.two_level = 0;  // one level beyond 16 384 tiles: a single counter copy, no sample
    CHECK(tile_run(layout(20000, 20100), plan(20100, f), A, many, many).path == TilePath::DirectRounds);
    CHECK(tile_run(layout(20000, 20100), plan(20100, f), A, many, many).sample == 1);
    // the forces: S where a sample can run, and only there; k
    TileForces g;
    g.fused_scan = 0;
    g.sample_stride = 4;
    g.sample_k = 0;
    CHECK(tile_run(layout(50, 52), plan(52, g), A, 10, 10).sample == 4 && tile_run(layout(50, 52), plan(52, g), A, 10, 10).sample_k == 0);
    g.sample_stride = 1;
    CHECK(tile_run(layout(4888, 4890), plan(4890, g), A, many, many).sample == 1);
    g.sample_stride = 1000;  // (no more than 16)
    CHECK(tile_run(layout(4888, 4890), plan(4890, g), A, many, many).sample == 16);
    g.fused_scan = 1;
    CHECK(tile_run(layout(50, 52), plan(52, g), A, 10, 10).path == TilePath::Fused && tile_run(layout(50, 52), plan(52, g), A, 10, 10).sample == 1);
}

// Which slots of a range a sampled count takes (tile_sample_first / tile_sample_step: the arithmetic k_tile_count walks
// with): wave w of W has the range's slots w, w + W, ...; of those exactly the j-th with (j + w) % S == 0.
static void walk() {
    for (uint32_t W : {16u, 8u})
        for (uint32_t S : {2u, 4u, 8u, 16u})
            for (uint32_t len : {1u, 2u, 15u, 16u, 17u, 18u, 34u, 255u, 256u, 257u, 5086u}) {
                std::vector<int> picked(len, 0);
                for (uint32_t w = 0; w < W; ++w) {
                    CHECK(tile_sample_first(w, W, S) % W == w && tile_sample_first(w, W, S) < W * S);
                    for (uint32_t q = tile_sample_first(w, W, S); q < len; q += tile_sample_step(W, S)) ++picked[q];
                }
                uint32_t n = 0;
                for (uint32_t q = 0; q < len; ++q) {
                    CHECK(picked[q] == (((q / W) + (q % W)) % S == 0 ? 1 : 0));  // once, and only those
                    n += picked[q];
                }
                CHECK(picked[0] == 1);                                 // a range's first slot is always in the sample
                if (len >= W * S) CHECK(n >= len / S - W && n <= len / S + W);  // one in S, give or take the ragged end
            }
    // S = 2, 16 waves: wave 1 skips its first slot and takes number 17; wave 0 takes 0 and 32
    CHECK(tile_sample_first(1, 16, 2) == 17 && tile_sample_first(0, 16, 2) == 0 && tile_sample_step(16, 2) == 32);
    CHECK(tile_sample_first(3, 16, 4) == 19 && tile_sample_first(15, 16, 16) == 31 && tile_sample_first(5, 16, 1) == 5);
}

// the sum of the capacities of `stretches` equal stretches whose estimates add up to `est` -- the worst case of the bound
static uint64_t caps_sum(uint64_t est, uint64_t stretches, uint32_t S, uint32_t k) {
    const uint64_t c = est / S / stretches;
    return stretches * tile_cap(static_cast<uint32_t>(c), S, k);
}

static void allocation() {
    // exact plans get the values and one more, as before
    CHECK(tile_bucket_entries(layout(50, 52), plan(52), 1000) == 1001);
    CHECK(tile_bucket_entries(layout(20000, 20100), plan(20100), 1ull << 30) == (1ull << 30) + 1);
    CHECK(tile_cap_slack(1000, 8, 1, 8) == 0);
    // the headline: 22.5 % more
    const uint64_t n = 1000000000ull, e = tile_bucket_entries(layout(4888, 4890), plan(4890), n);
    CHECK(e > n + 22 * (n / 100) && e < n + 23 * (n / 100));
    // capacities that just fit: equal stretches whose estimates add up to every value the file can have fit the allocation,
    // and so do they with the estimates' sum k standard deviations (sqrt(S n)) above it
    for (uint64_t values : {1000000000ull, 250000000ull, 16384ull * 8 * 4890}) {
        const uint64_t room = tile_bucket_entries(layout(4888, 4890), plan(4890), values);
        const uint32_t S = tile_run(layout(4888, 4890), plan(4890), TilePhase::A, values, values).sample;
        CHECK(S > 1);
        CHECK(caps_sum(values, 8ull * 4890, S, 8) <= room);
        CHECK(caps_sum(values + 8 * tile_isqrt_up(S * values), 8ull * 4890, S, 8) <= room);
        // ... and just do not: the first sampled count per stretch whose capacities pass the room stands for an estimate
        // beyond k deviations of the estimates' sum, and less than one per cent above the values -- the room is no larger
        // than the bound needs
        uint32_t c = static_cast<uint32_t>(values / S / (8ull * 4890));
        while (8ull * 4890 * tile_cap(c, S, 8) <= room) ++c;
        const uint64_t over = static_cast<uint64_t>(c) * S * 8ull * 4890;
        CHECK(8ull * 4890 * tile_cap(c - 1, S, 8) <= room);
        CHECK(over > values + 8 * tile_isqrt_up(S * values) && over < values + values / 100);
    }
    // a skewed stream needs less: all the estimate in one stretch
    CHECK(tile_cap(62500000u, 16, 8) + (8ull * 4890 - 1) * tile_cap(0, 16, 8) < tile_bucket_entries(layout(4888, 4890), plan(4890), n));
    // the allocation a test forces
    TileForces f;
    f.bucket_room = 777;
    CHECK(tile_bucket_entries(layout(4888, 4890), plan(4890, f), n) == 777);
    // 2^31 records: the entries still fit 32 bits
    CHECK(tile_bucket_entries(layout(4888, 4890), plan(4890), 0x7fffffffull) < 0xffffffffull);
}

int main() {
    roots();
    capacities();
    strides();
    walk();
    allocation();
    printf("tile sample plan: %d checks %s\n", g_checks, g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
