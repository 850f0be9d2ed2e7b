// Which bucketing kernels a layout runs in each phase, and with which tables: decided HERE and nowhere else.  The LDS tile
// histogram (tile_hist.hip) buckets a phase's values by bin tile -- count, scan, scatter -- and histograms every tile in LDS.
//   tiles of [uniq_cov2 | taxa]   phase A (over the bins' tiles alone)                  phase B
//   <= 4064                       Fused                                                 Fused
//   4065 .. 6144                  OrderedRounds                                         OrderedRounds
//   6145 .. 16384                 OrderedRounds (bins' tiles <= 6144) or DirectRounds   Matrix (values / tiles < 4096) or DirectRounds
//   16385 .. 36864                TwoLevel                                              Matrix (values / tiles < 4096) or TwoLevel
//   > 36864 (tile_tables_fit_lds), or SLIMM_FORCE direct_atomics: DirectAtomics in both
// Plain host C++, no HIP runtime and no context: tests/native/tile_plan_check.cpp walks the table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "force.h"

namespace slimm {

// The bins are cut into TILES of 2^shift consecutive bins; tile_hist.hip is compiled once per tile size into its own
// namespace (tiles13: 8192 bins, tiles14: 16384 bins -- what the 16-bit bucket entries hold beside the unique bit), and a
// context picks one per layout (tile_layout).  Smaller tiles: more workgroups of k_tile_hist per CU, faster histograms;
// larger tiles: half as many bucket frontiers, longer runs of one tile among neighbouring targets and so fewer returning
// atomics in the direct rounds of the scatter.
constexpr uint32_t kTileShiftSmall = 13, kTileShiftLarge = 14;
// Bucket entries per k_tile_hist work item (packed 16-bit counts: below 65536).  Hot tiles (a few present genomes take most of
// a sample's reads) are cut into items of this size, each adding its counts to global memory with atomics, and k_pack goes
// over them once more: 16384 / 32768 / 49152 at config 3: k_tile_hist 224 / 162 / 153 us, k_pack 46 / 27 / 17; config 5:
// 319 / 312 / 310 and 27 / 15 / 13
constexpr uint32_t kTileSub = 49152;
// ... of phase B's single-array histogram (32-bit counts): the reads that keep several targets meet in the few tiles of the
// taxon entries, and smaller items are more workgroups on those
constexpr uint32_t kTileSubB = 16384;
constexpr uint32_t kTileSubWide = 262144;   // ... of the wide form (32-bit counts): far more than kTileSub entries per tile
constexpr size_t kTileLdsMax = 144 * 1024;  // LDS histogram of tile ids in k_tile_count / k_tile_scatter
inline bool tile_tables_fit_lds(uint32_t ntiles) { return static_cast<size_t>(ntiles) * 4 <= kTileLdsMax; }
// tile_count: `reps` copies of rep_stride words, zero on entry (k_zero); workgroup b adds to copy b % reps.
// k_tile_scan sums the copies into tile_base and turns every copy into the start of its stretch inside the buckets,
// which k_tile_scatter (same grid) then fills through the copy's own cursors: 1/reps of the same-address atomics.
#ifndef SLIMM_TILE_REPS
#define SLIMM_TILE_REPS 8
#endif
constexpr uint32_t kTileReps = SLIMM_TILE_REPS;
constexpr uint32_t kScanStagedTiles = 16384;  // tiles whose counter copies k_tile_scan stages in LDS (one copy beyond)
constexpr uint32_t kBigRoundTiles = 6144;     // tiles whose rounds k_tile_scatter_big orders in LDS (the direct rounds beyond)
constexpr uint32_t kFusedScanTiles = 4064;    // (4096 table entries less the room three small arrays take: tile_hist.hip)

struct TileLayout {
    uint32_t tile_shift = kTileShiftSmall;  // log2 of the bins per tile: which build of tile_hist.hip runs
    uint64_t Bp = 0;                        // bins per coverage array, padded to whole tiles
    uint32_t ntiles = 0;                    // their tiles: phase A's
    uint32_t Tpad = 0, ntiles2 = 0;         // the selectors' taxa padded likewise; tiles of [uniq_cov2 | taxa]: phase B's
    uint32_t tile_bins() const { return 1u << tile_shift; }
};
// Tile size by layout: the small tiles while the whole bucketing fits the fused kernel's tile tables (their histograms
// run at twice the occupancy), the large ones beyond -- where the scatter's direct rounds pay a returning atomic per
// run of one tile among neighbouring targets and half as many tiles make those runs longer (1 B records over 20 k
// references: scatter 3.03 -> 2.3 ms, histograms 0.41 -> 0.67 ms).  forced_shift: SLIMM_FORCE tile_shift = 13 | 14
inline TileLayout tile_layout(uint64_t bins, uint32_t Tsel, long forced_shift = 0) {
    TileLayout l;
    const uint64_t small = (bins + (1ull << kTileShiftSmall) - 1) >> kTileShiftSmall;
    const uint64_t small2 = small + ((static_cast<uint64_t>(Tsel) + (1ull << kTileShiftSmall) - 1) >> kTileShiftSmall);
    l.tile_shift = small2 > kFusedScanTiles ? kTileShiftLarge : kTileShiftSmall;
    if (forced_shift == kTileShiftSmall || forced_shift == kTileShiftLarge) l.tile_shift = static_cast<uint32_t>(forced_shift);
    const uint32_t tb = l.tile_bins();
    l.Bp = (bins + tb - 1) & ~static_cast<uint64_t>(tb - 1);
    l.ntiles = static_cast<uint32_t>(l.Bp >> l.tile_shift);
    l.Tpad = (Tsel + tb - 1) & ~(tb - 1);
    l.ntiles2 = l.ntiles + (l.Tpad >> l.tile_shift);
    return l;
}

// What SLIMM_FORCE (force.h) says about the bucketing: read once, when the context is created
struct TileForces {
    bool direct_atomics = false;
    int two_level = -1;    // -1: by size, 0 / 1: never / always
    long fused_scan = 1;   // 0: the scan in a launch of its own
    long matrix = 1;       // 0: never, 2: always in phase B (small layouts too, whatever the number of values)
    long scatter_big = 1;  // 0: the direct rounds instead of the ordered ones
    int wide_tiles = -1;   // -1: by the file's size, 0 / 1: never / always
    long tile_shift = 0;   // 13 / 14
    static TileForces from_env() {
        TileForces f;
        long v = 0;
        f.direct_atomics = forced("direct_atomics");
        if (forced("two_level", &v)) f.two_level = v == 1;
        (void)forced("fused_scan", &f.fused_scan);
        (void)forced("matrix", &f.matrix);
        (void)forced("scatter_big", &f.scatter_big);
        if (forced("wide_tiles", &v)) f.wide_tiles = v == 1;
        (void)forced("tile_shift", &f.tile_shift);
        return f;
    }
};

struct TilePlan {  // of a layout: what holds for both phases
    bool use_tiles = false;         // LDS-privatised histograms (default) vs direct global atomics (too many tiles for LDS)
    bool two_level = false;         // bucket through super tiles first (many tiles: one-level scatter stores are too scattered)
    uint32_t reps = 1, stride = 0;  // copies of the tile counters / cursors and their stride
    bool fused = false;             // k_tile_scan runs inside the one-level bucketing kernel
    bool matrix_allowed = false;    // phase B may bucket through a count matrix (one row per counting workgroup, no atomics)
    bool matrix_always = false, scatter_big = true;
    int wide_tiles = -1;
};
// setup_ok: tile_hist_setup took the layout (it refuses what tile_tables_fit_lds refuses, and a failing HIP call)
inline TilePlan tile_plan(uint32_t ntiles2, const TileForces& f, bool setup_ok) {
    TilePlan p;
    p.use_tiles = !f.direct_atomics && setup_ok;
    // by size: with the register-resident scatter chunks one level wins up to ~10 K tiles (config 3: 494 vs 601 us) and is
    // level with two at 24 K (config 5: 430 vs 396 us)
    p.two_level = f.two_level >= 0 ? f.two_level == 1 : ntiles2 > kScanStagedTiles;
    if (!p.use_tiles) return p;
    p.reps = (p.two_level || ntiles2 > kScanStagedTiles) ? 1u : kTileReps;
    p.stride = ntiles2 + 1;
    p.fused = !p.two_level && p.reps == kTileReps && ntiles2 <= kFusedScanTiles && f.fused_scan != 0;
    // Layouts beyond the fused kernel's 4064 tiles, PHASE B only, when a tile gets few selectors (decided per file from the
    // number of reads): a count matrix instead of counter copies and cursors -- one row of tile counts per counting
    // workgroup, no global atomics and no rounds in the scatter.  (Phase A stays on the rounds: with hundreds of thousands
    // of values per tile, appending at ONE frontier per tile and counter copy keeps the bucket's open cache lines in L2,
    // while 256 private frontiers per tile -- 2.5 M partially written lines at config 3 -- turn every 2-byte store into a
    // partial-line write: measured 834 vs 362 us.)  Only beyond kBigRoundTiles tiles: up to there the rounds ordered by
    // tile in LDS (k_tile_scatter_big) are faster for both phases (config 3, phase B: count 28 -> 17 us, scatter 52 -> 42).
    p.matrix_allowed = !p.fused && f.matrix != 0 && (ntiles2 > kBigRoundTiles || f.matrix == 2);
    p.matrix_always = f.matrix == 2;
    p.scatter_big = f.scatter_big != 0;
    p.wide_tiles = f.wide_tiles;
    return p;
}

enum class TilePhase { A, B };
enum class TilePath {
    DirectAtomics,  // no bucketing: global atomics straight into the arrays (k_hist / k_sel_atomics)
    Fused,          // count, then ONE kernel that scans and scatters (and writes the histogram's work items)
    OrderedRounds,  // count, scan, k_tile_scatter_big: rounds ordered by tile in LDS, whole runs appended per tile
    DirectRounds,   // count, scan, k_tile_scatter: a returning atomic per run of one tile among neighbouring values
    Matrix,         // count into a row per workgroup, column prefix, scan of the sums, k_tile_scatter_matrix: no atomics
    TwoLevel        // count, scan, k_part_super (by super tile into `mid`), k_part_tile (by tile inside a super tile)
};
// the tables (tile_bucketing.h) a path uses: tile_count, tile_base, tile_cursor, tile_items + split_tiles, bucket,
// tile_matrix, {mid, part_items, sup_cursor}
enum TileTable : uint32_t { kTabCount = 1, kTabBase = 2, kTabCursor = 4, kTabItems = 8, kTabBucket = 16, kTabMatrix = 32, kTabSuper = 64 };
struct TileRun {  // the path of a phase and what depends on it
    TilePhase phase = TilePhase::A;
    TilePath path = TilePath::DirectAtomics;
    uint32_t ntiles = 0;           // the phase's tiles
    uint32_t scan_reps = 1;        // k_tile_scan: the copies it sums (Matrix: the one row of column sums) ...
    bool scan_two_level = false;   // ... and whether it also lays out the super tiles
    uint32_t tile_sub = kTileSub;  // entries per work item of k_tile_hist
    bool wide_hist = false;        // k_tile_hist with 32-bit counts for two arrays (phase B's one array has them anyway)
    uint32_t tables = 0, zeroed = 0;  // TileTable bits: what the path uses, and what of it is zero when its first kernel starts
};
// values: the phase's values (phase A: a target per record at most; phase B: a selector per read); records: the file's
inline TileRun tile_run(const TileLayout& l, const TilePlan& p, TilePhase phase, uint64_t values, uint64_t records) {
    TileRun r;
    const bool B = phase == TilePhase::B;
    r.phase = phase;
    r.ntiles = B ? l.ntiles2 : l.ntiles;
    if (!p.use_tiles) return r;
    // few selectors per tile (config 5: 100; config 3: 1 200): the count matrix (88 -> 61 us at config 3, 112 -> 33 us at
    // config 5); many (config 4: 12 000): the direct rounds, whose shared frontier per tile keeps the open lines in L2
    const bool matrix = B && p.matrix_allowed && (p.matrix_always || values / std::max(1u, l.ntiles2) < 4096u);
    // (the plan is made for phase B's tiles: phase A's may still fit the ordered rounds when those do not)
    const bool ordered = p.scatter_big && p.reps > 1 && r.ntiles <= kBigRoundTiles;
    r.path = p.fused ? TilePath::Fused : matrix ? TilePath::Matrix : p.two_level ? TilePath::TwoLevel
             : ordered ? TilePath::OrderedRounds : TilePath::DirectRounds;
    r.scan_reps = matrix ? 1u : p.reps;
    r.scan_two_level = !matrix && p.two_level;
    // far more entries per tile than a packed work item holds (1 B records on 20 k references): work items of up to
    // kTileSubWide entries with 32-bit counts, so that a tile is one item again
    const bool wide = p.wide_tiles >= 0 ? p.wide_tiles != 0 : (l.ntiles && records / l.ntiles > 32768u);
    r.tile_sub = wide ? kTileSubWide : (B ? kTileSubB : kTileSub);
    r.wide_hist = wide && !B;
    r.tables = kTabCount | kTabItems | kTabBucket | (p.fused ? 0u : kTabBase) | (matrix ? kTabMatrix : kTabCursor) |
               (r.path == TilePath::TwoLevel ? kTabSuper : 0u);
    r.zeroed = kTabCount | (p.fused ? kTabCursor : 0u);  // (otherwise k_tile_scan clears the cursors)
    return r;
}

}  // namespace slimm
