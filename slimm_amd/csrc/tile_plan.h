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

// ---- the sampled count (OrderedRounds and DirectRounds with kTileReps counter copies) ----
// k_tile_count may count every S-th slot (dense form: piece) only; k_tile_scan then gives every (copy, tile) stretch a
// CAPACITY instead of its count, the scatter fills the stretches as ever, and k_tile_fit compares every fill with its
// capacity: one stretch too small and the whole bucketing runs again with S = 1 (tile_bucketing.hip).  A 1-in-S thinning
// of n entries estimates n with a standard deviation of sqrt(S n) -- at the TRUE n, which is what has to be bounded: the
// largest n that lies within k deviations of the estimate S c solves (n - S c)^2 = k^2 S n, so
//   cap(c) = S (c + k^2 / 2 + k sqrt(c + k^2 / 4)) + S      (c: the sampled count; k: kSampleK standard deviations)
// With the variance taken at the estimate instead (S c + k sqrt(S (S c + S)) + S, the first form of this rule) the large
// stretches had their k deviations and the small ones did not: a stretch of 145 entries of which a 1-in-16 sample saw none
// overran cap(0) = 144 with probability 9e-5, and the headline has 39 K stretches (profiles/round17: the fullest stretch at
// 0.98 of its capacity).  Now cap(0) = S k^2 + S = 1040 at S = 16, which 1040 entries miss with probability (15/16)^1040 =
// 7e-30.  At S entries of the estimate per 1024 of the stretch (kSamplePerStride) the head-room is 29 % at most.
#if defined(__HIPCC__)
#define SLIMM_HD __host__ __device__
#else
#define SLIMM_HD
#endif
constexpr uint32_t kSampleMaxStride = 16;
constexpr uint32_t kSampleK = 8;
constexpr uint32_t kSamplePerStride = 1024;  // values per (copy, tile) and unit of S below which S is halved
// Values a sample has to leave unread to be worth its risk: the sampled chain costs k_tile_fit, three launches that return
// at once and a longer scan -- about 45 us a phase -- and the count reads 4 bytes per value at 5.2 TB/s.  Asked for: TWICE
// that cost in skipped bytes, 112 M values = 86 us.  Measured (profiles/round17): config 3, phase A, 100 M values at S = 2
// lost 16 us a step; the headline's phase B, 119 M selectors at S = 2, was level (-42 us of count, +53 of chain) and keeps
// the full count with both; its phase A, 1 B at S = 16, skips 937 M.
constexpr uint64_t kSampleMinSkipped = 112000000ull;
SLIMM_HD inline uint64_t tile_isqrt_up(uint64_t x) {  // the least r with r * r >= x (x < 2^62); host: the allocation's bound
    uint64_t r = static_cast<uint64_t>(__builtin_sqrt(static_cast<double>(x)));
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r * r < x ? r + 1 : r;
}
SLIMM_HD inline uint32_t tile_isqrt_up32(uint32_t x) {  // the same in 32 bits (x < 2^31): what k_tile_scan takes per stretch
    uint32_t r = static_cast<uint32_t>(__builtin_sqrtf(static_cast<float>(x)));  // (a first guess: the loops make it exact)
    while (r * r > x) --r;
    while ((r + 1u) * (r + 1u) <= x) ++r;
    return r * r < x ? r + 1u : r;
}
// the capacity of a stretch whose sample counted c: S c + S k^2 / 2 + k S ceil(sqrt(4 c + k^2)) / 2 (rounded up) + S; k <= 64.
// Never above 0xffffffff (c from 2^28 on: the sum then cannot fit any allocation, and k_tile_scan, which adds the
// capacities up in 64 bits, says so)
SLIMM_HD inline uint32_t tile_cap(uint32_t c, uint32_t S, uint32_t k) {
    if (c >= (1u << 28)) return 0xffffffffu;
    const uint32_t r = tile_isqrt_up32(4u * c + k * k);  // < 2^15
    const uint64_t cap = static_cast<uint64_t>(S) * c + (S * k * k + 1u) / 2u + (k * S * r + 1u) / 2u + S;
    return cap > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(cap);
}
// Which slots (dense form: pieces) of a counting workgroup's range a sampled count takes.  Wave w of the workgroup's W
// walks the range's slots w, w + W, w + 2 W, ...: its j-th is sampled when (j + w) % S == 0, so every wave has a share of
// the sample.  first: the wave's first sampled slot of the range, step: from one sampled slot to its next.
SLIMM_HD inline uint32_t tile_sample_first(uint32_t wave, uint32_t waves, uint32_t S) { return wave + waves * ((S - wave % S) % S); }
SLIMM_HD inline uint32_t tile_sample_step(uint32_t waves, uint32_t S) { return waves * S; }
// S for `values` values at most over ntiles tiles and kTileReps copies: the largest power of two <= kSampleMaxStride that
// leaves kSamplePerStride values per (copy, tile) and unit of S; 1 = count everything (fewer than 2048 per stretch).
// `values` is what the host knows before the launch -- phase A: the file's RECORDS, of which 0.62 are targets at the
// headline (15.8 K per stretch where S = 16 asks for 16 K) -- and an average: a skewed file has stretches of a few hundred
// entries beside the full ones.  Neither matters to whether a stretch fits, which tile_cap holds at any size; they move
// the head-room spent (k sqrt(S / n) of a stretch of n) up a little.
inline uint32_t tile_sample_stride(uint64_t values, uint32_t ntiles) {
    const uint64_t per = values / (static_cast<uint64_t>(kTileReps) * std::max(1u, ntiles));
    uint32_t S = kSampleMaxStride;
    while (S > 1 && per < static_cast<uint64_t>(kSamplePerStride) * S) S >>= 1;
    return S;
}
// Bucket entries beyond the values themselves that the capacities of `stretches` stretches may take.  The estimates S c
// add up to the values give or take sqrt(S values): est = values + k of those.  The roots ceil(sqrt(4 c + k^2)) add up to
// at most sqrt(stretches * (4 est / S + k^2 stretches)) + stretches (Cauchy-Schwarz, and the rounding), so
//   sum(cap) <= est + (k S / 2) (that) + (S k^2 / 2 + S + 2) stretches.
// A sum that does not fit after all is one more reason for the exact fallback, never an overrun.
inline uint64_t tile_cap_slack(uint64_t values, uint64_t stretches, uint32_t S, uint32_t k) {
    if (S <= 1) return 0;
    const uint64_t est = values + k * tile_isqrt_up(S * values);
    const uint64_t roots = tile_isqrt_up(stretches * (4 * est / S + 4 + static_cast<uint64_t>(k) * k * stretches)) + stretches;
    return (est - values) + (static_cast<uint64_t>(k) * S * roots + 1) / 2 + (static_cast<uint64_t>(S) * k * k / 2 + S + 2) * stretches;
}

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
    long sample_stride = 0;  // 0: by size; 1: always the full count; 2 .. 16: this S wherever a sampled count can run
    long sample_k = -1;      // -1: kSampleK
    long bucket_room = 0;    // > 0: the bucket allocation holds this many entries whatever the file (a test of the capacities'
                             // sum against it; it has to hold the file's values)
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
        (void)forced("sample_stride", &f.sample_stride);
        (void)forced("sample_k", &f.sample_k);
        (void)forced("bucket_room", &f.bucket_room);
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
    uint32_t sample_stride = 0, sample_k = kSampleK;  // TileForces: 0 = by size
    uint64_t bucket_room = 0;
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
    p.sample_stride = static_cast<uint32_t>(std::min<long>(std::max<long>(f.sample_stride, 0), kSampleMaxStride));
    if (f.sample_k >= 0) p.sample_k = static_cast<uint32_t>(std::min<long>(f.sample_k, 64));
    p.bucket_room = f.bucket_room > 0 ? static_cast<uint64_t>(f.bucket_room) : 0;
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
    uint32_t sample = 1;           // S of the count: 1 = every value (today's chain), > 1 = sampled, capacities, k_tile_fit
    uint32_t sample_k = kSampleK;
};
// whether a run may count a sample at all: the rounds whose bases and cursors come from k_tile_scan, with all the copies
// (Fused scans inside its scatter, Matrix needs exact rows, TwoLevel exact super tiles, DirectAtomics has no buckets)
inline bool tile_path_samples(const TilePlan& p, TilePath path, uint32_t ntiles) {
    return (path == TilePath::OrderedRounds || path == TilePath::DirectRounds) && p.reps == kTileReps && ntiles <= kScanStagedTiles;
}
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
    r.sample_k = p.sample_k;
    if (tile_path_samples(p, r.path, r.ntiles))
        r.sample = p.sample_stride ? p.sample_stride : tile_sample_stride(values, r.ntiles);
    if (!p.sample_stride && r.sample > 1 && values - values / r.sample < kSampleMinSkipped) r.sample = 1;
    return r;
}

// Entries of the bucket allocation for a file of n records (no more values than that in either phase): the values, one
// more, and the head-room of the sampled capacities -- at 1 B records over 4 888 tiles of 8 copies, S = 16, k = 8: 22.5 % more
// (0.45 GB).  k_tile_scan gets this number as the allocation the capacities have to fit.
inline uint64_t tile_bucket_entries(const TileLayout& l, const TilePlan& p, uint64_t n) {
    if (p.bucket_room) return p.bucket_room;
    uint64_t slack = 0;
    for (TilePhase ph : {TilePhase::A, TilePhase::B}) {
        const TileRun r = tile_run(l, p, ph, n, n);
        slack = std::max(slack, tile_cap_slack(n, static_cast<uint64_t>(kTileReps) * r.ntiles, r.sample, r.sample_k));
    }
    return n + 1 + slack;
}

}  // namespace slimm
