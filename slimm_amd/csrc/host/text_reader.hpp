// A compressed stream's text, decoded serially on the host: what the readers of gzip, bzip2, zstd and xz SAM have in common.
// A decoder says how the next piece of text is made (next_text); the buffer of compressed bytes it is made from and the
// hand-out of the text in pieces of the caller's size are here, once.  Header-only: every decoder is compiled on its own by
// some test program.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace slimm {

class TextReader {
public:
    // `source(dst, cap)`: the next compressed bytes of the file, in order (0 at its end)
    using Source = std::function<size_t(uint8_t*, size_t)>;
    explicit TextReader(Source source) : source_(std::move(source)) {}
    virtual ~TextReader() = default;
    // the next decoded bytes, at most `cap` -- fewer only at the end of the last stream --; 0 at that end, -1 + error()
    long read(uint8_t* dst, size_t cap) {
        size_t out = 0;
        while (!bad_ && out < cap) {
            if (served_ >= text_.size()) {
                if (done_ || !next_text()) break;
                continue;
            }
            const size_t n = std::min(cap - out, text_.size() - served_);
            memcpy(dst + out, text_.data() + served_, n);
            served_ += n;
            out += n;
        }
        return bad_ ? -1 : static_cast<long>(out);
    }
    // the decoder's own words: "block at byte N: <cause>", ... (without what the file's reader puts in front)
    const std::string& error() const { return err_; }

protected:
    // more text into text_, behind or in place of what has been served (false: the end -- done_ --, or err_ and bad_)
    virtual bool next_text() = 0;
    // at least n bytes at pos_ (false: the file has no more)
    bool need(size_t n) {
        while (in_.size() - pos_ < n && !in_eof_) {
            if (pos_ > (1u << 20)) {   // (the bytes in front of the one being read are done with)
                in_.erase(in_.begin(), in_.begin() + static_cast<long>(pos_));
                in_base_ += pos_;
                pos_ = 0;
            }
            const size_t have = in_.size(), chunk = 4u << 20;
            in_.resize(have + chunk);
            const size_t got = source_(in_.data() + have, chunk);
            in_.resize(have + got);
            if (got == 0) in_eof_ = true;
        }
        return in_.size() - pos_ >= n;
    }
    Source source_;
    std::vector<uint8_t> in_;   // compressed bytes from file offset in_base_ on; the next to read: pos_
    uint64_t in_base_ = 0;
    size_t pos_ = 0;
    bool in_eof_ = false, done_ = false, bad_ = false;
    std::vector<uint8_t> text_;   // decoded text (and what the decoder keeps of it to copy from)
    size_t served_ = 0;           // ... of which [served_, size) have not been handed out
    std::string err_;
};

}  // namespace slimm
