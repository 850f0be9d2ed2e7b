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
bool all_zero(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

}  // namespace

bool XzReader::fail(const std::string& where, uint32_t status, const std::string& more) {
    err_ = where + ": " + xz::status_text(status) + more;
    bad_ = true;
    return false;
}

// behind a block's end marker: the padding, the sizes against the header's, the check
bool XzReader::end_block() {
    const std::string where = "block at byte " + std::to_string(block_at_);
    const uint32_t pad = static_cast<uint32_t>((4u - ((bh_.bytes + block_comp_) & 3u)) & 3u), cb = xz::check_bytes(check_);
    if (!need(pad + cb)) return fail(where, xz::kRanOut);
    const uint8_t* p = in_.data() + pos_;
    if (!all_zero(p, pad)) return fail(where, xz::kBadBlockPadding);
    if ((bh_.has_compressed && bh_.compressed != block_comp_) || (bh_.has_uncompressed && bh_.uncompressed != block_text_))
        return fail(where, xz::kBadBlockSizes);
    if (check_ == xz::kCheckCrc32) {
        if (xz::le32(p + pad) != ~static_cast<uint32_t>(crc_)) return fail(where, xz::kBadCheck);
        ++n_.check_crc32;
    } else if (check_ == xz::kCheckCrc64) {
        if (xz::le64(p + pad) != ~crc_) return fail(where, xz::kBadCheck);
        ++n_.check_crc64;
    } else {
        ++(check_ == xz::kCheckSha256 ? n_.sha256_unverified : n_.check_none);
    }
    pos_ += pad + cb;
    records_.emplace_back(bh_.bytes + block_comp_ + cb, block_text_);
    ++n_.blocks;
    stage_ = Stage::Stream;
    return true;
}

// the index and the footer behind it
bool XzReader::read_index() {
    const std::string where = "index at byte " + std::to_string(in_base_ + pos_);
    uint64_t count = 0, first = 0, bytes = 0;
    uint32_t st;
    while ((st = xz::index_extent(in_.data() + pos_, in_.size() - pos_, &count, &first, &bytes)) == xz::kRanOut && need(in_.size() - pos_ + 1)) {
    }
    if (st != xz::kOk) return fail(where, st);
    if (count != records_.size()) return fail(where, xz::kIndexMismatch);
    uint64_t at = first;
    for (const auto& r : records_) {
        uint64_t unpadded = 0, uncompressed = 0;
        xz::index_record(in_.data() + pos_, bytes, &at, &unpadded, &uncompressed);
        if (unpadded != r.first || uncompressed != r.second) return fail(where, xz::kIndexMismatch);
    }
    n_.index_records += count;
    pos_ += bytes;
    const std::string foot = "stream footer at byte " + std::to_string(in_base_ + pos_);
    if (!need(xz::kHeaderBytes)) return fail(foot, xz::kRanOut);
    uint64_t stated = 0;
    st = xz::stream_footer(in_.data() + pos_, check_, &stated);
    if (st == xz::kOk && stated != bytes) st = xz::kBadFooter;
    if (st != xz::kOk) return fail(foot, st);
    pos_ += xz::kHeaderBytes;
    stage_ = Stage::Between;
    return true;
}

bool XzReader::next_text() {
    auto at = [&](size_t pos) { return std::to_string(in_base_ + pos); };
    for (;;) {
        if (stage_ == Stage::Between) {
            while (n_.streams > 0 && need(4) && all_zero(in_.data() + pos_, 4)) pos_ += 4;   // (stream padding)
            if (!need(xz::kHeaderBytes)) {
                const size_t left = in_.size() - pos_;
                if (left == 0 && n_.streams > 0) {
                    done_ = true;
                    return false;
                }
                const uint8_t* p = in_.data() + pos_;
                if (n_.streams == 0 || xz::magic_prefix(p, left)) return fail("stream header at byte " + at(pos_), xz::kRanOut);
                return fail("at byte " + at(pos_), all_zero(p, left) ? xz::kBadPadding : xz::kTrailing);
            }
            const uint8_t* p = in_.data() + pos_;
            if (!xz::is_magic(p)) return fail("at byte " + at(pos_), n_.streams > 0 && p[0] == 0 ? xz::kBadPadding : xz::kTrailing);
            const uint32_t st = xz::stream_header(p, &check_);
            if (st != xz::kOk) return fail("stream header at byte " + at(pos_), st);
            pos_ += xz::kHeaderBytes;
            records_.clear();
            ++n_.streams;
            stage_ = Stage::Stream;
            continue;
        }
        if (stage_ == Stage::Stream) {
            if (!need(1)) return fail("block header at byte " + at(pos_), xz::kRanOut);
            if (in_[pos_] == 0) {
                if (!read_index()) return false;
                continue;
            }
            uint32_t st;
            while ((st = xz::block_header(in_.data() + pos_, in_.size() - pos_, bh_)) == xz::kRanOut && need(in_.size() - pos_ + 1)) {
            }
            if (st == xz::kBadFilter) return fail("block header at byte " + at(pos_), st, " (filter id " + std::to_string(bh_.filter_id) + ")");
            if (st != xz::kOk) return fail("block header at byte " + at(pos_), st);
            block_at_ = in_base_ + pos_;
            pos_ += bh_.bytes;
            block_comp_ = block_text_ = since_ = 0;
            crc_ = ~0ull;
            rules_ = xz::Rules{};
            if (served_ == text_.size()) {   // (a block needs nothing of the one in front)
                text_.clear();
                served_ = 0;
            }
            stage_ = Stage::Chunks;
            continue;
        }
        // a chunk
        const std::string where = "chunk at byte " + at(pos_);
        xz::Chunk ch;
        uint32_t st;
        while ((st = xz::chunk_header(in_.data() + pos_, in_.size() - pos_, rules_, ch)) == xz::kRanOut && need(in_.size() - pos_ + 1)) {
        }
        if (st != xz::kOk) return fail(where, st);
        if (ch.control == 0) {
            ++pos_;
            ++block_comp_;
            if (!end_block()) return false;
            continue;
        }
        if (!need(ch.header + static_cast<size_t>(ch.csize))) return fail(where, xz::kRanOut);
        // (the text kept: the dictionary in front of this chunk)
        const uint64_t keep = std::min<uint64_t>(bh_.dict_size, since_);
        if (served_ == text_.size() && text_.size() > keep + (8u << 20)) {
            text_.erase(text_.begin(), text_.end() - static_cast<long>(keep));
            served_ = text_.size();
        }
        const size_t before = text_.size();
        text_.resize(before + ch.usize);
        uint8_t* out = text_.data() + before;
        const uint8_t* p = in_.data() + pos_;
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
            st = rc.init(p, ch.header, ch.header + static_cast<uint64_t>(ch.csize));
            if (st == xz::kOk) st = xz::lzma_chunk(rc, lz_, probs_.data(), out, ch.usize, since_, bh_.dict_size, t);
            if (st != xz::kOk) {
                text_.resize(before);
                return fail(where, st);
            }
            n_.match_bytes += t.match_bytes;
            n_.max_dist = t.max_dist;
        }
        crc_ = step(check_, crc_, out, ch.usize);
        since_ += ch.usize;
        block_text_ += ch.usize;
        block_comp_ += ch.header + static_cast<uint64_t>(ch.csize);
        n_.text += ch.usize;
        pos_ += ch.header + static_cast<size_t>(ch.csize);
        return true;
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
        if (all_zero(foot, 4)) {   // (stream padding)
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
