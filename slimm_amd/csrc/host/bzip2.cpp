// bzip2 on the host (bzip2.hpp): streams, blocks and their checks, serially.
#include "bzip2.hpp"

#include <cstring>

namespace slimm {

Bzip2Reader::Bzip2Reader(Source source) : TextReader(std::move(source)), tables_(new bz2::Tables) {
    bz2::crc_table(crc_tab_);
}
Bzip2Reader::~Bzip2Reader() { delete tables_; }

long Bzip2Reader::fail(const std::string& why) {
    err_ = why;
    bad_ = true;
    return -1;
}

bool Bzip2Reader::more_input() {
    pos_ = static_cast<size_t>(bit_ >> 3);   // (the byte being read: what lies in front of it may go)
    const uint64_t base = in_base_;
    const bool more = need(in_.size() - pos_ + 1);
    bit_ -= (in_base_ - base) * 8u;
    return more;
}

bool Bzip2Reader::next_text() {
    auto at = [&](uint64_t bit) { return std::to_string(in_base_ + (bit >> 3)); };
    for (;;) {
        if (!in_stream_) {   // a stream header, at a byte
            while (in_.size() - (bit_ >> 3) < 4 && more_input()) {
            }
            const size_t avail = in_.size() - static_cast<size_t>(bit_ >> 3);
            const uint8_t* h = in_.data() + (bit_ >> 3);
            if (avail == 0 && streams_ > 0) {
                done_ = true;
                return false;
            }
            if (avail < 4 || memcmp(h, "BZh", 3) != 0 || h[3] < '1' || h[3] > '9') {
                const bool prefix = avail < 4 && memcmp(h, "BZh", avail) == 0;
                fail(prefix ? "truncated stream header at byte " + at(bit_)
                            : streams_ ? "bytes after the last end-of-stream marker, at byte " + at(bit_) : "not a bzip2 stream");
                return false;
            }
            level_ = static_cast<uint32_t>(h[3] - '0');
            combined_ = 0;
            in_stream_ = true;
            ++streams_;
            bit_ += 32;
        }
        while (in_.size() * 8u - bit_ < 80u && more_input()) {
        }
        bz2::Bits b(in_.data(), bit_, in_.size() * 8u);
        uint64_t magic;
        if (!b.peek48(magic)) {
            fail("truncated at byte " + at(bit_));
            return false;
        }
        if (magic == bz2::kEosMagic) {
            uint32_t v, hi, lo;
            if (!b.get(24, v) || !b.get(24, v) || !b.get(16, hi) || !b.get(16, lo)) {
                fail("truncated end-of-stream marker at byte " + at(bit_));
                return false;
            }
            if (((hi << 16) | lo) != combined_) {
                fail("end-of-stream marker at byte " + at(bit_) + ": combined CRC mismatch");
                return false;
            }
            bit_ = (b.pos() + 7u) & ~7ull;
            in_stream_ = false;
            continue;
        }
        if (magic != bz2::kBlockMagic) {
            fail("at byte " + at(bit_) + ": " + bz2::status_text(bz2::kNoBlock));
            return false;
        }
        const uint32_t max_n = level_ * 100000u;
        if (tt_.size() < max_n) tt_.resize(max_n);
        if (ll_.size() < max_n) ll_.resize(max_n);
        uint32_t counts[256];
        bz2::BlockInfo info;
        uint32_t st;
        for (;;) {
            st = bz2::decode_block(in_.data(), bit_, in_.size() * 8u, max_n, *tables_, ll_.data(), counts, info);
            if (st == bz2::kRanOut && more_input()) continue;
            break;
        }
        if (st != bz2::kOk) {
            fail("block at byte " + at(bit_) + ": " + bz2::status_text(st));
            return false;
        }
        // inverse BWT from origPtr, then RLE1 undone into text_, the text's CRC checked
        uint32_t cf[256];
        bz2::link_block(ll_.data(), info.n, counts, tt_.data(), cf);
        text_.clear();
        served_ = 0;
        uint32_t crc = 0xffffffffu, p = info.orig_ptr;
        bz2::Rle1 r;
        for (uint32_t k = 0; k < info.n; ++k) {
            const uint32_t u = tt_[p];
            uint32_t byte;
            const uint32_t copies = r.step(u >> 24, byte);
            p = u & bz2::kLinkMask;
            for (uint32_t c = 0; c < copies; ++c) {
                text_.push_back(static_cast<uint8_t>(byte));
                crc = bz2::crc_byte(crc_tab_, crc, byte);
            }
        }
        if (r.count_missing()) {   // (four equal bytes end the block and no count byte follows: bzip2 refuses it too)
            fail("block at byte " + at(bit_) + ": " + bz2::status_text(bz2::kBadRun));
            return false;
        }
        if (~crc != info.crc) {
            fail("block at byte " + at(bit_) + ": " + bz2::status_text(bz2::kBadCrc));
            return false;
        }
        combined_ = ((combined_ << 1) | (combined_ >> 31)) ^ info.crc;
        bit_ = info.end_bit;
        return true;
    }
}

}  // namespace slimm
