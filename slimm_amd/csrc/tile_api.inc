// Declarations of tile_hist.hip's entry points -- included by kernels.h inside namespace tiles13 and namespace tiles14
// (no include guard: once per tile size).  The launch_tile_* are called by the driver alone (tile_bucketing.hip), which
// takes the kernels of a TilePath (tile_plan.h); `t` are the tables (kernels.h: TileTables).
int tile_hist_setup(uint32_t ntiles);                   // 0 = usable for this many tiles
uint32_t tile_count_grid(uint32_t grid);
uint32_t part_items_upper(uint32_t ntiles, uint32_t n_upper);
uint32_t tile_items_upper(uint32_t ntiles, uint32_t n_upper);
// totals: also one partial sum {mapped records, reads, targets} per workgroup into t.tot_part (kernels.h: Totals).
// matrix: instead of adding to a copy of t.tile_count, every counting workgroup stores one ROW of counts
// (tile_count_grid(grid) rows of t.stride words in t.matrix) ...
// sm (kernels.h: TileSample): stride > 1 counts every stride-th slot (dense: piece) of a workgroup's range, the totals still
// over all its slots; gated: nothing unless the phase's fallback flag is set
void launch_tile_count(hipStream_t st, uint32_t grid, uint32_t ntiles, const SlotValues& in, const TileTables& t, bool totals,
                       bool matrix, const TileSample& sm = TileSample());
// ... launch_matrix_prefix makes every column its exclusive prefix over the rows and leaves the column sums in
// t.tile_count (which launch_tile_scan then scans with reps = 1)
void launch_matrix_prefix(hipStream_t st, uint32_t grid, uint32_t ntiles, const TileTables& t);
// sm.stride > 1: the stretches get tile_cap() of their sampled counts, no work items are cut (launch_tile_fit does that),
// and counters[sm.flag] = whether the capacities' sum exceeds t.entries
void launch_tile_scan(hipStream_t st, uint32_t ntiles, const TileTables& t, uint32_t reps, bool two_level, const Totals& tot,
                      uint32_t tile_sub, const TileSample& sm = TileSample());
// bucketing by tile, by the path's kernel; also zeroes the tiles (of cov, and of ucov when given) that k_tile_hist will
// accumulate with atomics.
//   Fused: one-level with k_tile_scan folded in (<= kFusedScanTiles tiles, kTileReps copies of the counters): after
//     launch_tile_count, with t.tile_cursor zero; also writes k_tile_hist's work items, the split-tile list and their counts
//   OrderedRounds / DirectRounds: one level, k_tile_scatter_big / k_tile_scatter
//   Matrix: same grid as the count, places every value at tile_base[tile] + its row's prefix + a running LDS count: no
//     global atomics, no rounds
//   TwoLevel: k_part_super + k_part_tile
// sm (OrderedRounds / DirectRounds): the bucket stores are clamped to the allocation's last entry; behind a sampled count
// no tile is zeroed here (launch_tile_fit, which knows the fills, does it)
void launch_tile_scatter(hipStream_t st, TilePath path, uint32_t grid, uint32_t ntiles, uint32_t n_upper, const SlotValues& in,
                         const TileTables& t, uint32_t* cov, uint32_t* ucov, const Totals& tot, uint32_t tile_sub,
                         const TileSample& sm = TileSample());
// Behind the scatter of a sampled count: a fill above its capacity (the next stretch's start) raises
// counters[sm.flag] -- and clears t.tile_count for the exact chain that follows; otherwise the work items of k_tile_hist are
// cut from the real fills, {tile, lo, hi, pieces} with lo / hi counted over the tile's entries (its stretches' fills one
// behind the other), the split tiles listed and zeroed.  (The gated scan writes its items in the same form.)
void launch_tile_fit(hipStream_t st, uint32_t ntiles, const TileTables& t, uint32_t* cov, uint32_t* ucov, uint32_t tile_sub,
                     const TileSample& sm);
// stats != nullptr: k_tile_hist also accumulates the per-reference statistics {sum a, non-zero a, sum b, non-zero b}
// (stats[ref * 4 ..], zeroed by the caller) of the finished arrays; t.tile_ref0[tile] = first reference overlapping the
// tile (n_refs when none does).  For tiles cut into pieces only the sums are final; launch_pack adds their non-zero
// counts.  bits: also the 'bin != 0' bitmaps of the two arrays; finished tiles below store_from are not written out
// (their statistics are still taken)
// stretched: the items are launch_tile_fit's -- an item's entries lie in up to t.reps stretches (starts in t.tile_count, fills
// in t.tile_cursor) with gaps between them
void launch_tile_hist(hipStream_t st, uint32_t ntiles, uint32_t n_upper, const TileTables& t, uint32_t* cov, uint32_t* ucov,
                      const uint32_t* bin_off, uint32_t n_refs, uint32_t* stats, const BitsLayout& bits, uint32_t store_from,
                      bool wide, bool stretched = false);
// small arrays copied back to back to dst; with t and stats != nullptr also the non-zero bin counts of the tiles k_tile_hist
// accumulated in pieces (t->split_tiles[0 .. t->counters[CNT_SPLIT])), read back from the finished arrays a / b
void launch_pack(hipStream_t st, uint32_t* dst, const PackArgs& pack, const TileTables* t = nullptr, const uint32_t* a = nullptr,
                 const uint32_t* b = nullptr, const uint32_t* bin_off = nullptr, uint32_t n_refs = 0, uint32_t* stats = nullptr,
                 const BitsLayout& bits = BitsLayout());
