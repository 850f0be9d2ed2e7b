// lzip on the host (lzip.hpp): members and their trailers, serially.
#include "lzip.hpp"

#include <algorithm>
#include <cstring>

namespace slimm {

bool LzipReader::fail(const std::string& words) {
    err_ = words;
    bad_ = true;
    return false;
}

// the members are the walker's (../lzip_walk.h); here: the bytes it asks for, what a member decodes to, and its CRC32
bool LzipReader::next_text() {
    using W = lzip::Walker;
    for (;;) {
        const bool at_end = in_eof_;
        const W::Item it = walk_.peek(in_.data() + pos_, in_.size() - pos_, in_base_ + pos_, at_end);
        if (it.kind == W::More) {
            if (at_end) return fail(it.words());
            walk_.take(it);   // (the search's cursor)
            need(it.want);
            continue;   // (at the file's end the next peek says what these bytes are)
        }
        if (it.kind == W::Error) return fail(it.words());
        if (it.kind == W::MayEnd) {
            if (need(1)) continue;
            done_ = true;
            return false;
        }
        const lzip::Trailer& tr = it.trailer;
        if (!lzip::text_fits_stream(tr.data_size, it.bytes - lzip::kHeaderBytes - lzip::kTrailerBytes) || tr.data_size > 0xffffffffull)
            return fail(it.where() + ": " + lzip::status_text(lzip::kMarkerEarly));
        text_.clear();
        served_ = 0;
        text_.resize(static_cast<size_t>(tr.data_size));
        probs_.assign(lzip::kProbs, xz::kProbInit);
        xz::Tally t{0, 0};
        const uint8_t* p = in_.data() + pos_;
        uint8_t none = 0;
        const uint32_t st = lzip::lzma_member(p, lzip::kHeaderBytes, it.bytes - lzip::kTrailerBytes, probs_.data(), text_.empty() ? &none : text_.data(),
                                              static_cast<uint32_t>(tr.data_size), it.dict_size, t);
        if (st != lzip::kOk) return fail(it.where() + ": " + lzip::status_text(st));
        uint32_t c = 0xffffffffu;
        static uint32_t table[256];
        static const bool made = [] {
            for (uint32_t i = 0; i < 256u; ++i) table[i] = gz::crc_table_entry(i);
            return true;
        }();
        (void)made;
        for (uint8_t b : text_) c = table[(c ^ b) & 0xffu] ^ (c >> 8);
        if (~c != tr.crc) return fail(it.where() + ": " + lzip::status_text(lzip::kBadCrc));
        ++n_.members, ++n_.crc32_checked;
        if (text_.empty()) ++n_.empty_members;
        n_.match_bytes += t.match_bytes;
        n_.max_dist = std::max<uint64_t>(n_.max_dist, t.max_dist);
        n_.max_dict = std::max<uint64_t>(n_.max_dict, it.dict_size);
        n_.text += text_.size();
        walk_.take(it);
        pos_ += it.bytes;
        if (!text_.empty()) return true;
    }
}

bool lzip_read_index(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, std::vector<LzipIndexMember>* members) {
    members->clear();
    uint64_t end = size;
    while (end > 0) {
        uint8_t tail[lzip::kTrailerBytes], head[lzip::kHeaderBytes];
        if (end < lzip::kMemberMin || !read(end - lzip::kTrailerBytes, tail, lzip::kTrailerBytes)) return false;
        const lzip::Trailer tr = lzip::member_trailer(tail);
        if (tr.member_size < lzip::kMemberMin || tr.member_size > end) return false;
        const uint64_t at = end - tr.member_size;
        uint32_t dict = 0;
        if (!read(at, head, lzip::kHeaderBytes) || lzip::member_header(head, &dict) != lzip::kOk) return false;
        members->push_back(LzipIndexMember{at, tr.member_size, tr.data_size});
        end = at;
    }
    std::reverse(members->begin(), members->end());
    return !members->empty();
}

}  // namespace slimm
