// SLIMM_FORCE: the ONE environment variable by which tests and tuning runs make the library take a path it would not pick
// by itself -- the layout fallbacks of the tile kernels, the 32-byte lineage rows, a pair set that overflows, a grouping plan.
//   SLIMM_FORCE="key=value,key,key=value"      (a key without a value reads as 1)
// Read where a key is used -- the keys of the tile bucketing once, when a context is created (tile_plan.h: TileForces) -- so
// a test varies it between two contexts of one process.  Every key has a `-m gpu` test that names it:
//   direct_atomics, two_level=0|1, fused_scan=0, matrix=0|2, wide_tiles=0|1, tile_shift=13|14, scatter_big=0|1 (the tile
//   bucketing's: which path each takes a layout to is walked by tests/test_tile_plan.py), wide_rows, pair_cap=N
//                                                     tests/test_gpu_parity.py, test_gpu_layouts.py, test_gpu_group.py
//   group_bits=N, group_width=N, group_passes=N, group_grid=N, group_staged=0|1      tests/test_gpu_group_by_ident.py
//   group_collectives=rccl|copy                                                       tests/test_gpu_group.py
//   record_cap=N (fewer records per context), split_shift_guess (a mid-file member reports its first record one byte
//   off: slimm_group_stitch_ranges must refuse the join)                             tests/test_cli_split_input.py
//   bzip2_false_magics[=N] (block candidates that are no blocks: inside every real one, and every N bits), bzip2_round=N
//   (bzip2 SAM decoded every N compressed bytes: blocks cut across rounds)          tests/test_gpu_bzip2_sam.py
//   gzip_chunk=N (gzip SAM: a chunk start every N compressed bytes), gzip_round=N (decoded every N compressed bytes: blocks,
//   headers and trailers cut across rounds), gzip_false_starts[=N] (chunk starts that start no block: inside every real
//   one, and every N bits)                    tests/test_gpu_gzip_sam.py, tests/test_cli_gzip_sam_device.py
//   zstd_round=N (zstd SAM decoded every N compressed bytes: frame headers, block headers, blocks and checksums cut across
//   rounds), zstd_round_text=N (a round's text at most, by the blocks' bounds: copies reach into the history of an earlier
//   round)                                    tests/test_gpu_zstd_sam.py, tests/test_cli_zstd_sam_device.py,
//                                             tests/test_gpu_codec_paths.py (the directed inputs of tests/zstd_directed.py)
//   xz_round=N (xz SAM decoded every N compressed bytes: stream, block and chunk headers, chunks, checks, indexes and
//   footers cut across rounds), xz_round_text=N (a round's text at most: a round takes one block, the next round the
//   rest), xz_device_blocks=N (the `slimm` command reads an xz file of fewer than N blocks, by its index, on the host: 16
//   unless told)                              tests/test_gpu_xz_sam.py, tests/test_cli_xz_sam_device.py,
//                                             tests/test_gpu_codec_paths.py (xz_round, xz_round_text: the directed inputs of tests/lzma_directed.py)
//   lz4_round=N (lz4 SAM decoded every N compressed bytes: frame headers, block headers, blocks, end marks and checksums cut
//   across rounds), lz4_round_text=N (a round's text at most, by the blocks' bounds: with 65536 a round a block, so that a
//   linked frame's copies reach into the history of an earlier round)
//                                             tests/test_gpu_lz4_sam.py, tests/test_cli_lz4_sam_device.py
//   lzip_round=N (lzip SAM decoded every N compressed bytes: headers, streams and trailers cut across rounds, the member
//   finder fed a few bytes at a time), lzip_round_text=N (a round's text at most: a round takes one member, the next round
//   the rest), lzip_device_members=N (the `slimm` command reads an lzip file of fewer than N members, by its trailers, on
//   the host: 16 unless told)                 tests/test_gpu_lzip_sam.py, tests/test_cli_lzip_sam_device.py
//   xz_split_blocks=N (the least blocks per member at which the command cuts an xz file for --split-input: 16 unless told;
//   a key of its own, which does not follow xz_device_blocks)
//                                             tests/test_split_xz_ranges.py, tests/test_cli_split_input_xz.py
//   bzip2_split_wrong_first (a mid-file member of a split bzip2 file passes over its first block or marker:
//   slimm_group_stitch_ranges must refuse the cut)                                   tests/test_gpu_split_bzip2_sam.py
//   zstd_split_floor=N (the least bytes per member at which the command cuts a zstd file for --split-input: 32 MiB unless
//   told), zstd_cut_search=N (slimm_host_zstd_ranges gives a cut up N bytes behind its target: 64 MiB unless told),
//   zstd_split_wrong_cut (the planner's second cut -- of two members: its only one -- lands one byte late, where no frame
//   starts: the members or the stitch must refuse it)   tests/test_gpu_split_zstd_sam.py, tests/test_cli_split_input_zstd.py
//   gzip_split_floor=N (the least bytes per member at which the command cuts a gzip file for --split-input: 32 MiB unless
//   told), gzip_cut_blocks=N (slimm_host_gzip_ranges takes a block candidate for a cut when a walk from it passes N block
//   boundaries: 4 unless told), gzip_cut_search=N (... and gives a cut up N bytes behind its target: 64 MiB unless told),
//   gzip_split_wrong_cut (the planner's second cut -- of two members: its only one -- lands one bit late, where no block
//   starts: the members must refuse it)         tests/test_gpu_split_gzip_sam.py, tests/test_cli_split_input_gzip.py
//   sample_stride=S (the tile bucketing counts every S-th slot wherever a sampled count can run, 1: nowhere), sample_k=K
//   (standard deviations of head-room in a capacity: 8 unless told), bucket_room=N (the bucket allocation holds N entries
//   whatever the file: tile_plan.h)              tests/test_gpu_sampled_count.py, tests/test_tile_sample_plan.py
//   ref16=0 (the targets' reference words stay 32 bits wide on a database of at most 32 768 references, which takes the
//   16-bit form otherwise: kernels.h, TargetRefs)                                    tests/test_gpu_ref16.py
#pragma once
#include <cstdlib>
#include <cstring>

namespace slimm {

// true when SLIMM_FORCE names `key`; *text = its value's first character position (nullptr when it has none)
inline bool forced_text(const char* key, const char** text) {
    const char* e = getenv("SLIMM_FORCE");
    if (text) *text = nullptr;
    if (!e) return false;
    const size_t n = strlen(key);
    for (const char* p = e; *p;) {
        const char* end = strchr(p, ',');
        const size_t len = end ? static_cast<size_t>(end - p) : strlen(p);
        if (len >= n && memcmp(p, key, n) == 0 && (len == n || p[n] == '=')) {
            if (text && len > n) *text = p + n + 1;
            return true;
        }
        if (!end) break;
        p = end + 1;
    }
    return false;
}
inline bool forced(const char* key, long* value = nullptr) {
    const char* t = nullptr;
    if (!forced_text(key, &t)) return false;
    if (value) *value = t ? atol(t) : 1;
    return true;
}
// a key's forced value, or `fallback`: only a value of at least `least` counts (0: a floor, which 0 switches off; 1: a size
// or a count that 0 would make meaningless)
inline unsigned long long forced_or(const char* key, unsigned long long fallback, long least = 0) {
    long v = 0;
    return forced(key, &v) && v >= least ? static_cast<unsigned long long>(v) : fallback;
}

// the most records one context takes: below 2^31 (32-bit record indices), lower with SLIMM_FORCE record_cap=N
inline unsigned long long record_cap() {
    long v = 0;
    const unsigned long long cap = 0x7fffffffull;
    return (forced("record_cap", &v) && v > 0 && static_cast<unsigned long long>(v) < cap) ? static_cast<unsigned long long>(v) : cap;
}

// SLIMM_TRACE="cli,host,push" (or "all" / "1"): diagnostics on stderr -- cli: the command's stage marks (host/slimm_main.cpp),
// host: the library's host steps between the device phases (context.h: HostTrace), push: the window pipeline's events
// (windows.hip), tiles: which count placed the last file's buckets, when a context is destroyed (context.hip).  Nothing is
// computed differently with it.
inline bool traced(const char* what) {
    const char* e = getenv("SLIMM_TRACE");
    if (!e || !*e) return false;
    if (strcmp(e, "1") == 0 || strcmp(e, "all") == 0) return true;
    const size_t n = strlen(what);
    for (const char* p = e; *p;) {
        const char* end = strchr(p, ',');
        const size_t len = end ? static_cast<size_t>(end - p) : strlen(p);
        if (len == n && memcmp(p, what, n) == 0) return true;
        if (!end) break;
        p = end + 1;
    }
    return false;
}

}  // namespace slimm
