// The planner of slimm_host_gzip_ranges (split.hip): where a gzip-compressed SAM file is cut for the members of a group.
// Plain host C++ on deflate_stream.h's host-callable functions, without the HIP runtime, so that
// tests/native/san_gzip_plan.cpp can run it under the sanitizers.
// A deflate stream has no marks: a cut is a BIT at which a non-final dynamic block plausibly starts -- gz::is_candidate
// holds, and a walk from there (Huffman codes only, the text counted and thrown away) passes kGzipCutBlocks block
// boundaries, or a final block, without an error.  The walk reads at most kGzipCutWalk compressed bytes; when they run out
// the candidate counts if at least one boundary was passed.  Nothing the walk cannot see is trusted: a cut it took can still
// be false, and the members and the stitch decide (gzip_decode.hip: the rounds, split_gz_chains).
#pragma once
#include <memory>
#include <vector>

#include "deflate_stream.h"
#include "split_plan.h"

namespace slimm {

// stated defaults, not measurements (SLIMM_FORCE gzip_cut_blocks=N, gzip_cut_search=N bytes)
constexpr uint32_t kGzipCutBlocks = 4;
constexpr uint64_t kGzipCutSearch = 64ull << 20;
constexpr uint64_t kGzipCutWalk = 4ull << 20;
constexpr uint64_t kGzipCutScan = 1ull << 20;   // bytes whose bits are tried per read of the file

struct GzipPlan {
    uint32_t cut_blocks = kGzipCutBlocks;
    uint64_t cut_search = kGzipCutSearch;
};

// a walk from bit `bit` of p[0, end_byte): does a block chain start there?
inline bool gzip_walk_holds(const uint8_t* p, uint64_t bit, uint64_t end_byte, uint32_t cut_blocks, gz::Tables& t) {
    gz::Bits br(p, bit, end_byte);
    for (uint32_t passed = 0;;) {
        gz::Count out;
        bool fin = false;
        const uint32_t st = gz::inflate_block(br, t, out, &fin, nullptr);
        if (st == gz::kRanOut) return passed >= 1u;
        if (st != gz::kOk) return false;
        if (fin || ++passed >= cut_blocks) return true;
    }
}

// The bit behind the block that holds inflated byte skip - 1 (skip = 0: the first block's first bit), the file's members
// inflated from its first byte on.  false: no gzip member starts the file, or its text ends, or does not inflate, in
// front of that byte
template <typename Read>
bool gzip_header_end(Read&& read, uint64_t size, uint64_t skip, uint64_t* floor_bit) {
    std::vector<uint8_t> in;
    auto more = [&]() {   // the file's next bytes behind `in` (false: none left, or a read error)
        const uint64_t have = in.size(), add = std::min<uint64_t>(size - have, std::max<uint64_t>(1u << 20, have));
        if (!add) return false;
        in.resize(static_cast<size_t>(have + add));
        return read(have, in.data() + have, static_cast<size_t>(add));
    };
    std::unique_ptr<gz::Tables> t(new gz::Tables);
    uint64_t bit = 0, decoded = 0;
    for (;;) {   // a member
        const uint64_t at = bit >> 3;
        const long h = at <= in.size() ? gz::member_header(in.data() + at, in.size() - at) : 0;
        if (h < 0) return false;
        if (h == 0) {
            if (!more()) return false;
            continue;
        }
        bit = (at + static_cast<uint64_t>(h)) * 8u;
        if (decoded >= skip) break;   // (skip = 0, or a header that ends with a member)
        for (bool fin = false; !fin;) {   // its blocks
            gz::Bits br(in.data(), bit, in.size());
            gz::Count out;
            const uint32_t st = gz::inflate_block(br, *t, out, &fin, nullptr);
            if (st == gz::kRanOut) {
                fin = false;
                if (!more()) return false;
                continue;
            }
            if (st != gz::kOk) return false;
            bit = br.pos();
            decoded += out.n;
            if (decoded >= skip) break;
        }
        if (decoded >= skip) break;
        bit = ((bit + 7u) & ~7ull) + 64u;   // (the trailer: member 0 checks it)
    }
    *floor_bit = std::min(bit, size * 8u);
    return true;
}

// The first cut at or behind bit t, looked for in [t, t + cut_search bytes): kNoCut when there is none
template <typename Read>
uint64_t gzip_cut_at(Read&& read, uint64_t size, uint64_t t, const GzipPlan& plan, gz::Tables& tab, std::vector<uint8_t>& buf) {
    const uint64_t end_bit = size * 8u;
    if (t >= end_bit) return end_bit;
    const uint64_t stop = plan.cut_search < (end_bit - t) / 8u ? t + plan.cut_search * 8u : end_bit;
    for (uint64_t from = t; from < stop;) {
        const uint64_t at = from >> 3, n = std::min<uint64_t>(size - at, kGzipCutScan + kGzipCutWalk);
        buf.resize(static_cast<size_t>(n));
        if (!read(at, buf.data(), static_cast<size_t>(n))) return kNoCut;
        const uint64_t to = std::min(stop, (at + kGzipCutScan) * 8u);
        for (uint64_t b = from; b < to; ++b) {
            const uint64_t rel = b - at * 8u;
            if (!gz::cheap_candidate(buf.data(), rel, n) || !gz::is_candidate(buf.data(), rel, n, tab)) continue;
            if (gzip_walk_holds(buf.data(), rel, std::min<uint64_t>(n, (rel >> 3) + kGzipCutWalk), plan.cut_blocks, tab)) return b;
        }
        from = to;
    }
    return kNoCut;
}

// bits[0] = 0, bits[n] = 8 x size, the cuts in between; member i reads the file's bytes [bits[i] / 8, (bits[i + 1] + 7) / 8)
template <typename Read>
bool gzip_plan_ranges(Read&& read, uint64_t size, uint64_t skip, uint32_t n, uint64_t* bits, const GzipPlan& plan) {
    if (size >= (1ull << 60)) return false;
    uint64_t floor = 0;
    if (!gzip_header_end(read, size, skip, &floor)) return false;
    std::unique_ptr<gz::Tables> tab(new gz::Tables);
    std::vector<uint8_t> buf;
    uint64_t last_t = kNoCut, last_cut = kNoCut;   // (targets rise: a search that ends behind the next target answers it too)
    even_ranges(floor, size * 8u, n, bits, [&](uint64_t t) {
        if (last_t != kNoCut && t >= last_t && last_cut != kNoCut && t <= last_cut) return last_cut;
        last_t = t;
        last_cut = gzip_cut_at(read, size, t, plan, *tab, buf);
        return last_cut;
    });
    return true;
}

}  // namespace slimm
