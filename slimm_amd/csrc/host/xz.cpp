// xz on the host (xz.hpp): streams, blocks, LZMA2 chunks and their checks, serially.
#include "xz.hpp"

#include <algorithm>
#include <cstring>

#include "../split_plan.h"

namespace slimm {
namespace {

struct CrcTables {
    uint32_t t32[256];
    uint64_t t64[256];
    CrcTables() {
        for (uint32_t i = 0; i < 256u; ++i) t32[i] = gz::crc_table_entry(i), t64[i] = xz::crc64_table_entry(i);
    }
};
const CrcTables& tables() {
    static const CrcTables t;
    return t;
}
// the check's register (CRC32 in the low half) stepped over n bytes
uint64_t step(uint32_t check, uint64_t reg, const uint8_t* p, size_t n) {
    const CrcTables& t = tables();
    if (check == xz::kCheckCrc32) {
        uint32_t c = static_cast<uint32_t>(reg);
        for (size_t i = 0; i < n; ++i) c = t.t32[(c ^ p[i]) & 0xffu] ^ (c >> 8);
        return c;
    }
    if (check == xz::kCheckCrc64)
        for (size_t i = 0; i < n; ++i) reg = t.t64[(reg ^ p[i]) & 0xffu] ^ (reg >> 8);
    return reg;
}
}  // namespace

bool XzReader::fail(const std::string& words) {
    err_ = words;
    bad_ = true;
    return false;
}

// the container is the walker's (../xz_walk.h); here: the bytes it asks for, what its chunks decode to, and the checks
bool XzReader::next_text() {
    using W = xz::Walker;
    for (;;) {
        const W::Item it = walk_.peek(in_.data() + pos_, in_.size() - pos_, in_base_ + pos_);
        if (it.kind == W::More && need(it.want)) continue;
        if (it.kind == W::More || it.kind == W::Error) return fail(it.words());
        if (it.kind == W::MayEnd) {
            if (need(1)) continue;
            done_ = true;
            return false;
        }
        const uint8_t* p = in_.data() + pos_;
        const uint32_t check = walk_.check;
        bool text = false;
        if (it.kind == W::BlockStart) {
            since_ = 0;
            crc_ = ~0ull;
            if (served_ == text_.size()) {   // (a block needs nothing of the one in front)
                text_.clear();
                served_ = 0;
            }
        } else if (it.kind == W::BlockEnd) {   // (the check field behind the end marker and the padding)
            const uint8_t* field = p + 1u + it.pad;
            if (check == xz::kCheckCrc32 ? xz::le32(field) != ~static_cast<uint32_t>(crc_) : check == xz::kCheckCrc64 && xz::le64(field) != ~crc_) {
                return fail(it.where() + ": " + xz::status_text(xz::kBadCheck));
            }
            ++(check == xz::kCheckCrc32 ? n_.check_crc32 : check == xz::kCheckCrc64 ? n_.check_crc64 : check == xz::kCheckSha256 ? n_.sha256_unverified : n_.check_none);
            ++n_.blocks;
        } else if (it.kind == W::Index) {
            n_.index_records += it.count;
        } else if (it.kind == W::ChunkItem) {
            const xz::Chunk& ch = it.chunk;
            const uint32_t dict_size = walk_.block.bh.dict_size;
            // (the text kept: the dictionary in front of this chunk)
            const uint64_t keep = std::min<uint64_t>(dict_size, since_);
            if (served_ == text_.size() && text_.size() > keep + (8u << 20)) {
                text_.erase(text_.begin(), text_.end() - static_cast<long>(keep));
                served_ = text_.size();
            }
            const size_t before = text_.size();
            text_.resize(before + ch.usize);
            uint8_t* out = text_.data() + before;
            if (ch.dict_reset) since_ = 0;
            if (!ch.lzma) {
                memcpy(out, p + ch.header, ch.usize);
                ++n_.raw_chunks;
            } else {
                if (ch.new_props) {
                    lz_.lc = ch.lc, lz_.lp = ch.lp, lz_.pb = ch.pb;
                    ++n_.prop_changes;
                    if (ch.props != 0x5du) ++n_.odd_props;
                }
                if (ch.state_reset) {
                    lz_.reset_state();
                    probs_.assign(xz::n_probs(lz_.lc, lz_.lp), xz::kProbInit);
                    ++n_.state_resets;
                }
                ++n_.lzma_chunks;
                xz::Rc rc;
                xz::Tally t{0, static_cast<uint32_t>(n_.max_dist)};
                uint32_t st = rc.init(p, ch.header, ch.header + static_cast<uint64_t>(ch.csize));
                if (st == xz::kOk) st = xz::lzma_chunk(rc, lz_, probs_.data(), out, ch.usize, since_, dict_size, t);
                if (st != xz::kOk) {
                    text_.resize(before);
                    return fail(it.where() + ": " + xz::status_text(st));
                }
                n_.match_bytes += t.match_bytes;
                n_.max_dist = t.max_dist;
            }
            crc_ = step(check, crc_, out, ch.usize);
            since_ += ch.usize;
            n_.text += ch.usize;
            text = true;
        }
        walk_.take(it);
        n_.streams = walk_.streams;
        pos_ += it.bytes;
        if (text) return true;
    }
}

bool xz_read_index(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, std::vector<XzIndexBlock>* blocks, uint32_t* streams,
                   std::vector<XzIndexStream>* layout) {
    blocks->clear();
    *streams = 0;
    if (layout) layout->clear();
    std::vector<std::vector<XzIndexBlock>> per_stream;   // (the last stream first)
    std::vector<XzIndexStream> where;                    // (the same)
    uint64_t end = size;
    std::vector<uint8_t> index;
    while (end > 0) {
        uint8_t foot[xz::kHeaderBytes], head[xz::kHeaderBytes];
        if (end < 4u || (end & 3u) || !read(end - 4u, foot, 4)) return false;
        if (xz::all_zero(foot, 4)) {   // (stream padding)
            end -= 4u;
            continue;
        }
        if (end < 2u * xz::kHeaderBytes + 8u || !read(end - xz::kHeaderBytes, foot, xz::kHeaderBytes)) return false;
        uint64_t index_bytes = 0;
        if (xz::stream_footer(foot, foot[9], &index_bytes) != xz::kOk || index_bytes > end - 2u * xz::kHeaderBytes) return false;
        const uint64_t index_at = end - xz::kHeaderBytes - index_bytes;
        index.resize(index_bytes);
        if (!read(index_at, index.data(), index.size()) || index[0] != 0) return false;
        uint64_t count = 0, pos = 0, bytes = 0;
        if (xz::index_extent(index.data(), index.size(), &count, &pos, &bytes) != xz::kOk || bytes != index_bytes) return false;
        std::vector<XzIndexBlock> mine(count);
        uint64_t total = 0;
        for (XzIndexBlock& b : mine) {
            xz::index_record(index.data(), index.size(), &pos, &b.unpadded, &b.uncompressed);
            if (b.unpadded < 5u || b.unpadded > index_at) return false;
            b.at = total;   // (from the stream's first block on: the stream's start is not known yet)
            total += (b.unpadded + 3u) & ~3ull;
            if (total > index_at) return false;
        }
        if (index_at < total + xz::kHeaderBytes) return false;
        const uint64_t start = index_at - total - xz::kHeaderBytes;
        uint32_t check = 0;
        if (!read(start, head, xz::kHeaderBytes) || !xz::is_magic(head) || xz::stream_header(head, &check) != xz::kOk || check != foot[9]) return false;
        for (XzIndexBlock& b : mine) b.at += start + xz::kHeaderBytes;
        where.push_back(XzIndexStream{start, index_at + index_bytes + xz::kHeaderBytes, count, check});
        per_stream.push_back(std::move(mine));
        end = start;
    }
    if (per_stream.empty()) return false;
    *streams = static_cast<uint32_t>(per_stream.size());
    for (size_t s = per_stream.size(); s-- > 0;)
        for (XzIndexBlock& b : per_stream[s]) {
            b.stream = static_cast<uint32_t>(per_stream.size() - 1u - s);
            blocks->push_back(b);
        }
    if (layout) layout->assign(where.rbegin(), where.rend());
    return true;
}

bool xz_plan_ranges(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t skip, uint32_t n, uint64_t* offsets) {
    std::vector<XzIndexBlock> blocks;
    std::vector<XzIndexStream> layout;
    uint32_t streams = 0;
    return n && xz_read_index(read, size, &blocks, &streams, &layout) && xz_plan_ranges(blocks, layout, size, skip, n, offsets);
}

bool xz_plan_ranges(const std::vector<XzIndexBlock>& blocks, const std::vector<XzIndexStream>& layout, uint64_t size, uint64_t skip, uint32_t n,
                    uint64_t* offsets) {
    if (!n) return false;
    // no cut in front of the end of the block that holds decoded byte skip - 1: member 0 holds the whole header
    uint64_t first = 0, text = 0;
    for (size_t b = 0; skip && b < blocks.size() && text < skip; ++b) {
        text += blocks[b].uncompressed;
        first = blocks[b].at + ((blocks[b].unpadded + 3u) & ~3ull);
    }
    if (text < skip) return false;   // (the index states less text than that)
    std::vector<uint64_t> cuts;      // (in file order)
    size_t b = 0;
    for (const XzIndexStream& s : layout) {
        cuts.push_back(s.at);
        for (uint64_t k = 0; k < s.blocks; ++k, ++b)
            if (k) cuts.push_back(blocks[b].at);
    }
    cuts.push_back(size);
    even_ranges(first, size, n, offsets, [&](uint64_t t) { return *std::lower_bound(cuts.begin(), cuts.end(), std::min(t, size)); });
    return true;
}

bool xz_check_at(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t offset, int* check) {
    std::vector<XzIndexBlock> blocks;
    std::vector<XzIndexStream> layout;
    uint32_t streams = 0;
    if (!xz_read_index(read, size, &blocks, &streams, &layout)) return false;
    *check = -1;
    for (const XzIndexStream& s : layout)
        if (offset > s.at && offset < s.end) *check = static_cast<int>(s.check);
    return true;
}

}  // namespace slimm
