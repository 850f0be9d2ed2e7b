// The driver of the tile bucketing (tile_bucketing.h): the only caller of tile_hist.hip's launch_tile_*.  No kernel here.
#include "context.h"

namespace slimm {

const char* TileBucketing::init(const uint32_t* bin_off, uint32_t n_refs) {
    if (plan.matrix_allowed &&
        tile_matrix.ensure(static_cast<size_t>(TILES(layout.tile_shift, tile_count_grid(kGrid))) * plan.stride) != hipSuccess)
        return "the tile count matrix";
    const size_t rep_words = static_cast<size_t>(plan.reps) * plan.stride;
    if (tile_count.ensure(rep_words) != hipSuccess || tile_base.ensure(layout.ntiles2 + 1) != hipSuccess ||
        tile_cursor.ensure(rep_words) != hipSuccess || split_tiles.ensure(layout.ntiles2 + 1) != hipSuccess)
        return "tile tables";
    std::vector<uint32_t> ref0(layout.ntiles2 + 1, n_refs);
    uint32_t r = 0;
    for (uint32_t t = 0; t < layout.ntiles2; ++t) {
        const uint64_t t0 = static_cast<uint64_t>(t) * layout.tile_bins();
        if (t0 >= bin_off[n_refs]) break;
        while (r + 1 < n_refs && bin_off[r + 1] <= t0) ++r;
        ref0[t] = r;
    }
    if (d_tile_ref0.ensure(ref0.size()) != hipSuccess ||
        hipMemcpy(d_tile_ref0.p, ref0.data(), ref0.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return "tile tables";
    return nullptr;
}

hipError_t TileBucketing::reserve(uint32_t n) {
    hipError_t e = tot_part.ensure(kGrid);
    if (e != hipSuccess || !plan.use_tiles) return e;
    // (with the head-room of the sampled count's capacities, tile_plan.h; entry indices are 32-bit)
    entries = static_cast<uint32_t>(std::min<uint64_t>(tile_bucket_entries(layout, plan, n), 0xffffffffull));
    if ((e = bucket.ensure(entries)) != hipSuccess || (e = mid.ensure(n + 1)) != hipSuccess) return e;
    if ((e = tile_items.ensure(TILES(layout.tile_shift, tile_items_upper(layout.ntiles2, n)) + 1)) != hipSuccess) return e;
    if ((e = part_items.ensure(TILES(layout.tile_shift, part_items_upper(layout.ntiles2, n)) + 1)) != hipSuccess) return e;
    return sup_cursor.ensure(kMaxSuper);
}

static_assert(K_TILE_SCAN2 - K_TILE_COUNT2 == K_TILE_SCAN - K_TILE_COUNT && K_TILE_SCATTER2 - K_TILE_COUNT2 == K_TILE_SCATTER - K_TILE_COUNT,
              "phase B's timer ids follow phase A's in the same order");

// r.sample > 1 (tile_plan.h: the sampled count): the count over every S-th slot, the scan of capacities, the scatter, and
// k_tile_fit, which cuts the work items from the fills -- or, a stretch too small, raises the phase's fallback flag.  Behind
// it the exact chain (count, scan, scatter: its scan cuts the items in the fit's form) is launched whatever happened: each of its kernels looks at the flag and
// returns unless it is set, so there is no host round trip; a set flag makes it rewrite counts, bases, cursors, buckets and
// items from scratch.  The fit and the gated chain run under the scatter's timer id.
void bucket(slimm_ctx* c, const TileJob& job) {
    const TileRun& r = job.run;
    const TileTables t = c->tiles.tables(c->counters.p);
    const uint32_t grid = TileBucketing::kGrid;
    const int B = r.phase == TilePhase::B ? 1 : 0;
    const int id = B ? K_TILE_COUNT2 : K_TILE_COUNT;
    hipStream_t st = c->stream;
    const bool matrix = r.path == TilePath::Matrix;
    TileSample sm;
    sm.stride = r.sample;
    sm.k = r.sample_k;
    sm.flag = CNT_FALLBACK + B;
    c->tiles.sampled[B] = r.sample;
    {
        KernelTimer tm(c, id);
        TILES(t.tile_shift, launch_tile_count(st, grid, r.ntiles, job.values, t, job.tail != nullptr, matrix, sm));
        if (matrix) TILES(t.tile_shift, launch_matrix_prefix(st, grid, r.ntiles, t));
    }
    Totals tot;
    if (job.tail) tot = Totals{t.tot_part, TILES(t.tile_shift, tile_count_grid(grid)), job.tail};
    if (r.path != TilePath::Fused) {
        KernelTimer tm(c, id + (K_TILE_SCAN - K_TILE_COUNT));
        TILES(t.tile_shift, launch_tile_scan(st, r.ntiles, t, r.scan_reps, r.scan_two_level, tot, r.tile_sub, sm));
    }
    KernelTimer tm(c, id + (K_TILE_SCATTER - K_TILE_COUNT));
    TILES(t.tile_shift, launch_tile_scatter(st, r.path, grid, r.ntiles, job.n_upper, job.values, t, job.a, job.b, tot, r.tile_sub, sm));
    if (r.sample <= 1) return;
    TILES(t.tile_shift, launch_tile_fit(st, r.ntiles, t, job.a, job.b, r.tile_sub, sm));
    sm.stride = 1;
    sm.gated = true;  // (the totals are the first count's: published already)
    TILES(t.tile_shift, launch_tile_count(st, grid, r.ntiles, job.values, t, false, false, sm));
    TILES(t.tile_shift, launch_tile_scan(st, r.ntiles, t, r.scan_reps, r.scan_two_level, Totals(), r.tile_sub, sm));
    TILES(t.tile_shift, launch_tile_scatter(st, r.path, grid, r.ntiles, job.n_upper, job.values, t, job.a, job.b, Totals(), r.tile_sub, sm));
}

void histogram(slimm_ctx* c, const TileJob& job) {
    const TileRun& r = job.run;
    KernelTimer tm(c, r.phase == TilePhase::B ? K_TILE_HIST2 : K_TILE_HIST);
    const TileTables t = c->tiles.tables(c->counters.p);
    TILES(t.tile_shift, launch_tile_hist(c->stream, r.ntiles, job.n_upper, t, job.a, job.b, c->d_bin_off.p, c->R, job.stats, job.bits,
                                         job.store_from, r.wide_hist, r.sample > 1));
}

}  // namespace slimm
