// slimm_amd/csrc/tile_plan.h walked at the edges of its table: which bucketing path a layout of N tiles takes in each
// phase, under every SLIMM_FORCE key that moves it.  Stand-alone (g++, -fsanitize=address,undefined); built and run by
// tests/test_tile_plan.py.  The expectations are written out in numbers, not taken from the header's constants.
#include <cstdio>
#include <cstdlib>

#include "../../slimm_amd/csrc/tile_plan.h"

using namespace slimm;
using P = TilePath;

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
    l.ntiles = ntiles;
    l.ntiles2 = ntiles2;
    return l;
}
// the plan as slimm_create makes it: tile_hist_setup refuses when 4 bytes per tile exceed 144 KiB of LDS
static TilePlan plan(uint32_t ntiles2, const TileForces& f = TileForces()) {
    return tile_plan(ntiles2, f, static_cast<uint64_t>(ntiles2) * 4 <= 144u * 1024u);
}
static const uint64_t kMany = 1ull << 40;  // values: far more than 4096 per tile
static P path(uint32_t ntiles, uint32_t ntiles2, TilePhase ph, uint64_t values, const TileForces& f = TileForces()) {
    return tile_run(layout(ntiles, ntiles2), plan(ntiles2, f), ph, values, 0).path;
}

static void default_table() {
    const TilePhase A = TilePhase::A, B = TilePhase::B;
    for (uint32_t n : {1u, 4064u}) {  // row 1
        CHECK(path(n, n, A, kMany) == P::Fused && path(n, n, B, kMany) == P::Fused && path(n, n, B, 0) == P::Fused);
        const TilePlan p = plan(n);
        CHECK(p.use_tiles && p.fused && !p.two_level && p.reps == 8 && p.stride == n + 1 && !p.matrix_allowed);
        const TileRun r = tile_run(layout(n, n), p, B, 0, 0);
        CHECK(r.ntiles == n && (r.zeroed & kTabCursor) && (r.zeroed & kTabCount) && !(r.tables & (kTabMatrix | kTabSuper)));
    }
    for (uint32_t n : {4065u, 6144u}) {  // row 2: beyond the fused kernel, no matrix yet
        CHECK(path(n, n, A, kMany) == P::OrderedRounds && path(n, n, B, kMany) == P::OrderedRounds && path(n, n, B, 0) == P::OrderedRounds);
        const TileRun r = tile_run(layout(n, n), plan(n), B, 0, 0);
        CHECK(r.scan_reps == 8 && !r.scan_two_level && r.zeroed == kTabCount && (r.tables & kTabBase) && (r.tables & kTabCursor));
        CHECK(!plan(n).fused && !plan(n).matrix_allowed);
    }
    for (uint32_t n2 : {6145u, 16384u}) {  // row 3: phase A by ITS tiles, phase B by the values per tile
        CHECK(path(6144, n2, A, kMany) == P::OrderedRounds);
        CHECK(path(6145, n2, A, kMany) == P::DirectRounds);
        CHECK(path(n2 - 1, n2, B, 4095ull * n2 + n2 - 1) == P::Matrix);
        CHECK(path(n2 - 1, n2, B, 4096ull * n2) == P::DirectRounds);
        CHECK(path(6144, n2, A, 0) == P::OrderedRounds);  // (phase A never takes the matrix, however few its values)
        const TilePlan p = plan(n2);
        CHECK(p.reps == 8 && !p.two_level && p.matrix_allowed && !p.matrix_always);
        const TileRun m = tile_run(layout(n2 - 1, n2), p, B, 0, 0), d = tile_run(layout(n2 - 1, n2), p, B, kMany, 0);
        CHECK(m.scan_reps == 1 && !m.scan_two_level && (m.tables & kTabMatrix) && m.ntiles == n2);
        CHECK(d.scan_reps == 8 && !d.scan_two_level && !(d.tables & kTabMatrix));
    }
    for (uint32_t n2 : {16385u, 36864u}) {  // row 4
        CHECK(path(100, n2, A, kMany) == P::TwoLevel && path(n2 - 1, n2, A, kMany) == P::TwoLevel);
        CHECK(path(n2 - 1, n2, B, 4095ull * n2 + n2 - 1) == P::Matrix);
        CHECK(path(n2 - 1, n2, B, 4096ull * n2) == P::TwoLevel);
        const TilePlan p = plan(n2);
        CHECK(p.use_tiles && p.two_level && p.reps == 1 && p.stride == n2 + 1);
        const TileRun m = tile_run(layout(n2 - 1, n2), p, B, 0, 0), t = tile_run(layout(n2 - 1, n2), p, B, kMany, 0);
        CHECK(m.scan_reps == 1 && !m.scan_two_level && !(m.tables & kTabSuper));
        CHECK(t.scan_reps == 1 && t.scan_two_level && (t.tables & kTabSuper));
    }
    // row 5: the tile ids' LDS histogram does not fit
    CHECK(tile_tables_fit_lds(36864) && !tile_tables_fit_lds(36865));
    CHECK(!plan(36865).use_tiles);
    CHECK(path(36865, 36865, A, kMany) == P::DirectAtomics && path(36865, 36865, B, 0) == P::DirectAtomics);
    CHECK(tile_run(layout(36865, 36865), plan(36865), B, 0, 0).zeroed == 0);
}

static void forces() {
    const TilePhase A = TilePhase::A, B = TilePhase::B;
    TileForces f;
    f.fused_scan = 0;
    CHECK(path(90, 100, A, kMany, f) == P::OrderedRounds && path(90, 100, B, 0, f) == P::OrderedRounds);
    f.scatter_big = 0;
    CHECK(path(90, 100, A, kMany, f) == P::DirectRounds && path(90, 100, B, 0, f) == P::DirectRounds);
    f = TileForces();
    f.scatter_big = 0;  // (the fused kernel has no rounds to order)
    CHECK(path(90, 100, A, kMany, f) == P::Fused);
    CHECK(path(5000, 5000, A, kMany, f) == P::DirectRounds && path(5000, 5000, B, kMany, f) == P::DirectRounds);

    f = TileForces();
    f.two_level = 1;
    CHECK(path(90, 100, A, kMany, f) == P::TwoLevel && path(90, 100, B, 0, f) == P::TwoLevel);
    CHECK(plan(100, f).reps == 1 && plan(100, f).two_level && !plan(100, f).fused);
    CHECK(tile_run(layout(90, 100), plan(100, f), B, 0, 0).scan_two_level);
    f.two_level = 0;
    CHECK(path(20000, 20001, A, kMany, f) == P::DirectRounds && path(6000, 20001, A, kMany, f) == P::DirectRounds);  // (reps is 1)
    CHECK(path(20000, 20001, B, kMany, f) == P::DirectRounds && path(20000, 20001, B, 0, f) == P::Matrix);
    CHECK(plan(20001, f).reps == 1 && !plan(20001, f).two_level);

    f = TileForces();
    f.matrix = 2;
    CHECK(path(90, 100, B, kMany, f) == P::Fused);  // (the fused kernel goes first)
    f.fused_scan = 0;
    CHECK(path(90, 100, B, kMany, f) == P::Matrix && path(90, 100, B, 0, f) == P::Matrix);
    CHECK(path(90, 100, A, 0, f) == P::OrderedRounds);
    {
        const TileRun r = tile_run(layout(90, 100), plan(100, f), B, kMany, 0);
        CHECK(r.scan_reps == 1 && !r.scan_two_level && plan(100, f).reps == 8);
    }
    f.two_level = 1;  // (the matrix goes in front of the two levels, whose scan flag it drops)
    CHECK(path(90, 100, B, kMany, f) == P::Matrix && !tile_run(layout(90, 100), plan(100, f), B, kMany, 0).scan_two_level);
    f = TileForces();
    f.matrix = 0;
    CHECK(path(9999, 10000, B, 0, f) == P::DirectRounds && path(19999, 20000, B, 0, f) == P::TwoLevel);
    CHECK(!plan(10000, f).matrix_allowed && !plan(20000, f).matrix_allowed);

    f = TileForces();
    f.direct_atomics = true;
    CHECK(!plan(100, f).use_tiles && path(90, 100, A, kMany, f) == P::DirectAtomics && path(90, 100, B, 0, f) == P::DirectAtomics);
    CHECK(!tile_plan(100, TileForces(), false).use_tiles);  // tile_hist_setup failed
}

static void wide_items() {
    const TilePhase A = TilePhase::A, B = TilePhase::B;
    const TileLayout l = layout(10, 12);
    TileForces f;
    const TileRun a0 = tile_run(l, plan(12), A, 0, 32768ull * 10 + 9), b0 = tile_run(l, plan(12), B, 0, 32768ull * 10 + 9);
    CHECK(a0.tile_sub == 49152 && !a0.wide_hist && b0.tile_sub == 16384 && !b0.wide_hist);
    const TileRun a1 = tile_run(l, plan(12), A, 0, 32769ull * 10), b1 = tile_run(l, plan(12), B, 0, 32769ull * 10);
    CHECK(a1.tile_sub == 262144 && a1.wide_hist && b1.tile_sub == 262144 && !b1.wide_hist);
    f.wide_tiles = 0;
    CHECK(tile_run(l, plan(12, f), A, 0, 1ull << 31).tile_sub == 49152 && !tile_run(l, plan(12, f), A, 0, 1ull << 31).wide_hist);
    f.wide_tiles = 1;
    CHECK(tile_run(l, plan(12, f), A, 0, 0).tile_sub == 262144 && tile_run(l, plan(12, f), A, 0, 0).wide_hist);
    CHECK(tile_run(l, plan(12, f), B, 0, 0).tile_sub == 262144 && !tile_run(l, plan(12, f), B, 0, 0).wide_hist);
    CHECK(tile_run(layout(0, 1), plan(1), A, 0, 1ull << 31).tile_sub == 49152);  // no bins at all: nothing to divide by
}

static void layouts() {
    // small tiles while the 8192-bin tiles of [bins | taxa] number 4064 at most
    TileLayout l = tile_layout(4063ull * 8192, 8192);
    CHECK(l.tile_shift == 13 && l.tile_bins() == 8192 && l.Bp == 4063ull * 8192 && l.ntiles == 4063 && l.Tpad == 8192 && l.ntiles2 == 4064);
    l = tile_layout(4063ull * 8192 + 1, 8192);
    CHECK(l.tile_shift == 14 && l.tile_bins() == 16384 && l.Bp == 2032ull * 16384 && l.ntiles == 2032 && l.Tpad == 16384 && l.ntiles2 == 2033);
    l = tile_layout(4063ull * 8192 + 1, 8192, 13);
    CHECK(l.tile_shift == 13 && l.Bp == 4064ull * 8192 && l.ntiles == 4064 && l.ntiles2 == 4065);
    l = tile_layout(100, 5, 14);
    CHECK(l.tile_shift == 14 && l.Bp == 16384 && l.ntiles == 1 && l.Tpad == 16384 && l.ntiles2 == 2);
    l = tile_layout(100, 5, 12);  // (neither size: ignored)
    CHECK(l.tile_shift == 13 && l.Bp == 8192 && l.ntiles == 1 && l.Tpad == 8192 && l.ntiles2 == 2);
    l = tile_layout(0x7fff0000ull, 1);  // close to 2^31 bins: no 32-bit overflow on the way
    CHECK(l.tile_shift == 14 && l.Bp == 0x7fff0000ull && l.ntiles == 0x7fff0000u / 16384 && l.ntiles2 == l.ntiles + 1);
}

static void environment() {
    unsetenv("SLIMM_FORCE");
    TileForces f = TileForces::from_env();
    CHECK(!f.direct_atomics && f.two_level == -1 && f.fused_scan == 1 && f.matrix == 1 && f.scatter_big == 1 && f.wide_tiles == -1 && f.tile_shift == 0);
    setenv("SLIMM_FORCE", "two_level=0,matrix=2,scatter_big=0,wide_tiles,tile_shift=14,fused_scan=0,direct_atomics", 1);
    f = TileForces::from_env();
    CHECK(f.direct_atomics && f.two_level == 0 && f.fused_scan == 0 && f.matrix == 2 && f.scatter_big == 0 && f.wide_tiles == 1 && f.tile_shift == 14);
    setenv("SLIMM_FORCE", "two_level,wide_tiles=0,matrix=0", 1);
    f = TileForces::from_env();
    CHECK(!f.direct_atomics && f.two_level == 1 && f.wide_tiles == 0 && f.matrix == 0 && f.scatter_big == 1);
}

int main() {
    default_table();
    forces();
    wide_items();
    layouts();
    environment();
    if (g_failed) {
        fprintf(stderr, "tile plan: %d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("tile plan: %d checks ok\n", g_checks);
    return 0;
}
