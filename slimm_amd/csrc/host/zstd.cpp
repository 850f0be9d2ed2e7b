// zstd on the host (zstd.hpp): frames, blocks and their checks, serially.
#include "zstd.hpp"

#include <algorithm>
#include <cstring>

namespace slimm {

bool ZstdReader::fail(const std::string& where, uint32_t status) {
    err_ = where + ": " + zs::status_text(status);
    bad_ = true;
    return false;
}

uint32_t ZstdReader::decode_compressed(const uint8_t* content, uint32_t size, uint32_t block_max, uint64_t window, zs::Entropy& e, uint32_t rep[3],
                                       std::vector<uint8_t>& text, size_t frame_lo) {
    // the content, then what it repeats of the blocks in front (plan_compressed: aux), as one buffer
    std::vector<uint8_t> work(content, content + size), aux;
    work.insert(work.end(), zs::kPad, uint8_t(0));
    zs::Block b{};
    b.max = block_max;
    uint32_t st = zs::plan_compressed(work.data(), 0, size, e, aux, work.size(), b, nullptr);
    if (st != zs::kOk) return st;
    work.insert(work.end(), aux.begin(), aux.end());
    const uint8_t* base = work.data();
    std::vector<uint8_t> lit;
    const uint8_t* lits = nullptr;
    if (b.lit_type >= 2u) {
        uint8_t w[256];
        uint32_t n_w = 0, used = 0, log = 0, tmp[64];
        std::vector<uint16_t> table(1u << zs::kHufLogMax);
        st = zs::huf_read_weights(base + b.huf_at, b.huf_len, w, n_w, used, tmp);
        if (st == zs::kOk) st = zs::huf_build(w, n_w, table.data(), log);
        if (st != zs::kOk) return st;
        zs::LitStream s[4];
        st = zs::literal_streams(base, b, s);
        if (st != zs::kOk) return st;
        lit.resize(b.lit_regen + 1u);
        for (uint32_t k = 0; k < b.lit_streams; ++k) {
            st = zs::huf_decode_stream(base + s[k].at, s[k].len, table.data(), log, lit.data() + s[k].out, s[k].count);
            if (st != zs::kOk) return st;
        }
        lits = lit.data();
    } else if (b.lit_type == 1u) {
        lit.assign(b.lit_regen + 1u, base[b.lit_at]);
        lits = lit.data();
    } else {
        lits = base + b.lit_at;
    }
    std::vector<zs::Seq> seq(b.n_seq + 1u);
    uint32_t regen = b.lit_regen;
    seq[0] = zs::Seq{0, 0, 0};
    if (b.n_seq) {
        std::vector<uint32_t> tab(512u + 256u + 512u);
        uint32_t* const tables[3] = {tab.data(), tab.data() + 512, tab.data() + 768};
        uint32_t logs[3] = {0, 0, 0};
        for (uint32_t k = 0; k < 3u; ++k) {
            st = zs::seq_table(base, b.table[k], k, tables[k], logs[k]);
            if (st != zs::kOk) return st;
        }
        const zs::SeqTables t{{tables[0], tables[1], tables[2]}, {logs[0], logs[1], logs[2]}};
        st = zs::seq_decode(base + b.bits_at, b.bits_len, t, b.n_seq, b.lit_regen, block_max, seq.data(), rep, regen);
        if (st != zs::kOk) return st;
    } else if (regen > block_max) {
        return zs::kBlockTooLarge;
    }
    const size_t at = text.size();
    text.resize(at + regen);
    uint8_t* out = text.data() + at;
    for (uint32_t i = 0; i < b.n_seq; ++i) {
        const uint32_t ll = seq[i + 1].lit - seq[i].lit, ml = seq[i + 1].out - seq[i].out - ll, off = seq[i].off;
        memcpy(out + seq[i].out, lits + seq[i].lit, ll);
        const size_t m = at + seq[i].out + ll;
        if (off > window || off > m - frame_lo) return zs::kBadOffset;
        uint8_t* d = text.data() + m;
        for (uint32_t k = 0; k < ml; ++k) d[k] = d[static_cast<ptrdiff_t>(k) - static_cast<ptrdiff_t>(off)];
    }
    memcpy(out + seq[b.n_seq].out, lits + seq[b.n_seq].lit, b.lit_regen - seq[b.n_seq].lit);
    return zs::kOk;
}

bool ZstdReader::next_text() {
    auto at = [&](size_t pos) { return std::to_string(in_base_ + pos); };
    for (;;) {
        if (!in_frame_) {
            if (!need(4)) {
                if (in_.size() == pos_ && frames_ > 0) {
                    done_ = true;
                    return false;
                }
                const size_t left = in_.size() - pos_;
                return fail("at byte " + at(pos_), frames_ == 0 || zs::magic_prefix(in_.data() + pos_, left) ? zs::kRanOut : zs::kNoFrame);
            }
            const uint32_t magic = zs::le32(in_.data() + pos_);
            if ((magic & 0xfffffff0u) == zs::kSkippable) {
                if (!need(8)) return fail("skippable frame at byte " + at(pos_), zs::kRanOut);
                const size_t n = zs::le32(in_.data() + pos_ + 4);
                if (!need(8 + n)) return fail("skippable frame at byte " + at(pos_), zs::kRanOut);
                pos_ += 8 + n;
                ++frames_;
                continue;
            }
            if (magic != zs::kMagic) return fail("at byte " + at(pos_), frames_ ? zs::kNoFrame : zs::kRanOut);
            uint32_t st;
            while ((st = zs::frame_header(in_.data() + pos_, in_.size() - pos_, fh_)) == zs::kRanOut && need(in_.size() - pos_ + 1)) {
            }
            if (st != zs::kOk) return fail("frame header at byte " + at(pos_), st);
            frame_at_ = in_base_ + pos_;
            pos_ += fh_.bytes;
            in_frame_ = true;
            ++frames_;
            frame_len_ = 0;
            entropy_.reset();
            rep_[0] = 1, rep_[1] = 4, rep_[2] = 8;
            xxh_.reset();
            text_.clear();
            served_ = 0;
        }
        if (!need(3)) return fail("block header at byte " + at(pos_), zs::kRanOut);
        const uint32_t h = zs::le24(in_.data() + pos_), type = (h >> 1) & 3u, size = h >> 3;
        const bool last = h & 1u;
        const std::string where = "block at byte " + at(pos_);
        if (type == 3u) return fail(where, zs::kReservedBlock);
        if (size > fh_.block_max) return fail(where, zs::kBlockTooLarge);
        const size_t content = type == zs::kRleBlock ? 1u : size;
        if (!need(3 + content)) return fail(where, zs::kRanOut);
        // (the text kept: the window in front of this block)
        if (served_ == text_.size() && text_.size() > 2u * fh_.window + (1u << 20)) {
            text_.erase(text_.begin(), text_.end() - static_cast<long>(fh_.window));
            served_ = text_.size();
        }
        const size_t before = text_.size();
        const size_t frame_lo = frame_len_ >= before ? 0u : before - static_cast<size_t>(frame_len_);
        const uint8_t* p = in_.data() + pos_ + 3;
        if (type == zs::kRaw) text_.insert(text_.end(), p, p + size);
        else if (type == zs::kRleBlock)
            text_.insert(text_.end(), size, p[0]);
        else {
            const uint32_t st = decode_compressed(p, size, fh_.block_max, fh_.window, entropy_, rep_, text_, frame_lo);
            if (st != zs::kOk) return fail(where, st);
        }
        pos_ += 3 + content;
        xxh_.update(text_.data() + before, text_.size() - before);
        frame_len_ += text_.size() - before;
        if (last) {
            if (fh_.has_size && fh_.content_size != frame_len_) return fail("frame at byte " + std::to_string(frame_at_), zs::kBadContentSize);
            if (fh_.has_checksum) {
                if (!need(4)) return fail("checksum at byte " + at(pos_), zs::kRanOut);
                if (zs::le32(in_.data() + pos_) != static_cast<uint32_t>(xxh_.digest())) return fail("frame at byte " + std::to_string(frame_at_), zs::kBadChecksum);
                pos_ += 4;
            }
            in_frame_ = false;
        }
        if (text_.size() > before) return true;
    }
}

bool zstd_header_end(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t skip, uint64_t* end) {
    *end = 0;
    if (!skip) return true;
    uint64_t fed = 0;
    ZstdReader r([&](uint8_t* d, size_t cap) -> size_t {
        const size_t k = static_cast<size_t>(std::min<uint64_t>(cap, size - fed));
        if (!k || !read(fed, d, k)) return 0;
        fed += k;
        return k;
    });
    std::vector<uint8_t> buf(1u << 20);
    for (uint64_t left = skip; left;) {
        const long got = r.read(buf.data(), static_cast<size_t>(std::min<uint64_t>(left, buf.size())));
        if (got <= 0) return false;
        left -= static_cast<uint64_t>(got);
    }
    *end = r.file_pos();
    return !r.in_frame() || zs::walk_blocks(read, size, *end, r.frame().block_max, r.frame().has_checksum, end);
}

}  // namespace slimm
