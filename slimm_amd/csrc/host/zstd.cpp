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

// the container is the walker's (../zstd_walk.h); here: the bytes it asks for, and what its blocks decode to
bool ZstdReader::next_text() {
    for (bool any = false;;) {
        if (any && walk_.stage != zs::Walker::Checksum) return true;   // (a checksum behind the text is read with it)
        const zs::Walker::Item it = walk_.peek(in_.data() + pos_, in_.size() - pos_, in_base_ + pos_);
        if (it.kind == zs::Walker::More && need(it.want)) continue;
        if (it.kind == zs::Walker::More || it.kind == zs::Walker::Error) return fail(it.where(), it.status);
        if (it.kind == zs::Walker::MayEnd) {
            if (need(1)) continue;
            done_ = true;
            return false;
        }
        const std::string frame = zs::place_text(zs::Place::Frame, walk_.frame_at);
        if (it.kind == zs::Walker::Header) {
            frame_len_ = 0;
            entropy_.reset();
            rep_[0] = 1, rep_[1] = 4, rep_[2] = 8;
            xxh_.reset();
            text_.clear();
            served_ = 0;
        } else if (it.kind == zs::Walker::Sum) {
            if (it.sum != static_cast<uint32_t>(xxh_.digest())) return fail(frame, zs::kBadChecksum);
        } else if (it.kind == zs::Walker::Block) {
            const zs::FrameHeader& fh = walk_.fh;
            // (the text kept: the window in front of this block)
            if (served_ == text_.size() && text_.size() > 2u * fh.window + (1u << 20)) {
                text_.erase(text_.begin(), text_.end() - static_cast<long>(fh.window));
                served_ = text_.size();
            }
            const size_t before = text_.size();
            const size_t frame_lo = frame_len_ >= before ? 0u : before - static_cast<size_t>(frame_len_);
            const uint8_t* p = in_.data() + pos_ + 3;
            if (it.type == zs::kRaw) text_.insert(text_.end(), p, p + it.size);
            else if (it.type == zs::kRleBlock)
                text_.insert(text_.end(), it.size, p[0]);
            else {
                const uint32_t st = decode_compressed(p, it.size, fh.block_max, fh.window, entropy_, rep_, text_, frame_lo);
                if (st != zs::kOk) return fail(it.where(), st);
            }
            xxh_.update(text_.data() + before, text_.size() - before);
            frame_len_ += text_.size() - before;
            if (it.last && fh.has_size && fh.content_size != frame_len_) return fail(frame, zs::kBadContentSize);
            any = text_.size() > before;
        }
        walk_.take(it);
        pos_ += it.bytes;
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
