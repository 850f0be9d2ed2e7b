// The tile bucketing's state and its driver (tile_bucketing.hip): the layout and the plan of tile_plan.h, the tables that
// belong to them, and the two calls by which both phases run the kernels of a TilePath.  Included by context.h (DevBuf).
#pragma once

struct slimm_ctx;
namespace slimm {

struct TileBucketing {
    static constexpr uint32_t kGrid = 512;  // the bucketing grid: two persistent workgroups per CU
    TileLayout layout;
    TilePlan plan;
    TileRun run(TilePhase phase, uint64_t values, uint64_t records) const { return tile_run(layout, plan, phase, values, records); }

    DevBuf<uint16_t> bucket;           // targets bucketed by bin tile (the bin inside its tile | unique bit)
    uint32_t entries = 0;              // ... its entries as reserve() asked for them: what the sampled capacities have to fit
    uint32_t sampled[2] = {1, 1};      // the S of the last bucket() of phase A / B (slimm_get_bucket_sampling)
    DevBuf<uint32_t> tile_count, tile_base, tile_cursor, split_tiles, tile_matrix;
    DevBuf<uint4> tile_items, part_items;
    DevBuf<uint32_t> mid, sup_cursor;  // level-1 buckets (by super tile) and their cursors
    DevBuf<uint4> tot_part;            // per workgroup of k_tile_count: totals of its slots (kernels.h: Totals)
    DevBuf<uint32_t> d_tile_ref0;      // per bin tile: first reference overlapping it (fused statistics)

    // the tables sized by the layout, tile_ref0 from the references' first bins (bin_off[n_refs] = all bins); nullptr, or
    // what there was no device memory for
    const char* init(const uint32_t* bin_off, uint32_t n_refs);
    hipError_t reserve(uint32_t n_records);  // the tables sized by the file
    TileTables tables(uint32_t* counters) const {
        return TileTables{layout.tile_shift, bucket.p, tile_count.p, tile_base.p, tile_cursor.p, split_tiles.p, plan.reps, plan.stride,
                          tile_items.p, part_items.p, mid.p, sup_cursor.p, tile_matrix.p, tot_part.p, d_tile_ref0.p, counters, entries};
    }
    // what has to be zero when the run's first kernel starts, into the free entries of a phase's clearing launch
    void zero_tables(ZeroArgs& z, const TileRun& r) const {
        uint32_t i = 0;
        while (i < 5 && z.p[i]) ++i;
        if ((r.zeroed & kTabCount) && i < 5) z.p[i] = tile_count.p, z.n[i++] = plan.reps * plan.stride;
        if ((r.zeroed & kTabCursor) && i < 5) z.p[i] = tile_cursor.p, z.n[i++] = plan.reps * plan.stride;
    }
};

struct TileJob {  // one phase's bucketing and histogram: its values into the buckets by tile, the buckets into `a` (and `b`)
    TileRun run;  // TileBucketing::run of the phase
    SlotValues values;
    uint32_t n_upper = 0;            // the file's records: no more values than that
    uint32_t *a = nullptr, *b = nullptr;  // cov and uniq_cov, or uniq_cov2 alone (the taxa's counts behind it)
    uint32_t* tail = nullptr;        // != nullptr: the count also sums the stream's totals, the scan adds them up into the
                                     // counters and here (kernels.h: Totals)
    uint32_t* stats = nullptr;       // per-reference statistics of the finished arrays (tile_api.inc: the histogram), with bits and store_from
    BitsLayout bits;
    uint32_t store_from = 0;
};
// Two calls, because phase A has work of its own between them.  KernelTimer ids k_tile_count .. k_tile_hist (phase B: ...2)
void bucket(slimm_ctx* c, const TileJob& job);     // count (+ matrix prefix), scan unless fused, the scatter of the path
void histogram(slimm_ctx* c, const TileJob& job);  // k_tile_hist of the job's form

}  // namespace slimm
