// LZ4 on the host (lz4.hpp): frames, blocks and their checks, serially.
#include "lz4.hpp"

#include <algorithm>
#include <cstring>

namespace slimm {

bool Lz4Reader::fail(const std::string& where, uint32_t status) {
    err_ = where + ": " + lz4::status_text(status);
    bad_ = true;
    return false;
}

uint32_t Lz4Reader::decode_block(const uint8_t* p, uint32_t size, uint32_t block_max, std::vector<uint8_t>& text, size_t lo) {
    std::vector<lz4::Seq> seq;
    lz4::SeqWalk w;
    while (w.state < lz4::SeqWalk::Done) {
        if (w.pos >= size) return w.ran_off();
        lz4::Seq e[3];
        const uint32_t n = w.step(p[w.pos], size, e);
        seq.insert(seq.end(), e, e + n);
    }
    if (w.state == lz4::SeqWalk::Failed) return w.status;
    if (w.out > block_max) return lz4::kTextTooLarge;
    const size_t at = text.size();
    text.resize(at + w.out);
    for (size_t i = 0; i + 1u < seq.size(); ++i) {
        const lz4::Seq& s = seq[i];
        const uint32_t len = seq[i + 1u].out - s.out, ll = s.off == lz4::kLiteralsOnly ? len : s.off >> 16;
        memcpy(text.data() + at + s.out, p + s.lit, ll);
        if (ll == len) continue;
        const size_t m = at + s.out + ll, off = s.off & 0xffffu;
        if (off > m - lo) return lz4::kBadOffset;
        uint8_t* d = text.data() + m;
        for (uint32_t k = 0; k < len - ll; ++k) d[k] = d[static_cast<ptrdiff_t>(k) - static_cast<ptrdiff_t>(off)];
    }
    return lz4::kOk;
}

// the container is the walker's (../lz4_walk.h); here: the bytes it asks for, and what its blocks decode to
bool Lz4Reader::next_text() {
    using Walk = lz4::Walker;
    for (bool any = false;;) {
        if (any) return true;
        const Walk::Item it = walk_.peek(in_.data() + pos_, in_.size() - pos_, in_base_ + pos_);
        if (it.kind == Walk::More && need(it.want)) continue;
        if (it.kind == Walk::More || it.kind == Walk::Error) return fail(it.where(), it.status);
        if (it.kind == Walk::MayEnd) {
            if (need(1)) continue;
            done_ = true;
            return false;
        }
        const std::string frame = lz4::place_text(lz4::Place::Frame, walk_.frame_at);
        if (it.kind == Walk::Header) {
            frame_len_ = 0;
            xxh_.reset();
            text_.clear();
            served_ = 0;
        } else if (it.kind == Walk::EndMark) {
            if (walk_.fh.has_size && walk_.fh.content_size != frame_len_) return fail(frame, lz4::kBadContentSize);
        } else if (it.kind == Walk::Sum) {
            if (it.sum != xxh_.digest()) return fail(frame, lz4::kBadChecksum);
        } else if (it.kind == Walk::Block) {
            const lz4::FrameHeader& fh = walk_.fh;
            // (the text kept: the 64 KiB in front of this block)
            if (served_ == text_.size() && text_.size() > 2u * lz4::kHistory + (1u << 20)) {
                text_.erase(text_.begin(), text_.end() - static_cast<long>(lz4::kHistory));
                served_ = text_.size();
            }
            const size_t before = text_.size();
            const size_t lo = !fh.linked ? before : frame_len_ >= before ? 0u : before - static_cast<size_t>(frame_len_);
            const uint8_t* p = in_.data() + pos_ + 4;
            if (fh.block_sums && it.sum != lz4::xxh32(p, it.size)) return fail(it.where(), lz4::kBadBlockChecksum);
            if (it.stored) text_.insert(text_.end(), p, p + it.size);
            else {
                const uint32_t st = decode_block(p, it.size, fh.block_max, text_, lo);
                if (st != lz4::kOk) return fail(it.where(), st);
            }
            xxh_.update(text_.data() + before, text_.size() - before);
            frame_len_ += text_.size() - before;
            any = text_.size() > before;
        }
        walk_.take(it);
        pos_ += it.bytes;
    }
}

}  // namespace slimm
