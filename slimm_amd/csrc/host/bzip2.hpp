// bzip2 on the host: one serial decoder for the SAM header of a bzip2-compressed SAM file, for `--host-decode` and
// `--dump-records` / `--dump-raw` (the reader thread), and for the CPU tests.  The block decode is ../bzip2_block.h, the
// device decoder's own source; streams back to back (pbzip2, lbzip2) are read one after the other.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../bzip2_block.h"

namespace slimm {

class Bzip2Reader {
public:
    // `source(dst, cap)`: the next compressed bytes of the file, in order (0 at its end)
    explicit Bzip2Reader(std::function<size_t(uint8_t*, size_t)> source);
    ~Bzip2Reader();
    // the next decoded bytes, at most `cap`; 0 at the end of the last stream, -1 + error()
    long read(uint8_t* dst, size_t cap);
    // "block at byte N: <cause>", "truncated at byte N", ... (without the reader's "bzip2-compressed input ..." in front)
    const std::string& error() const { return err_; }

private:
    bool next_block();   // decode the next block into out_ (false: the end, or err_)
    bool more_input();   // false: the file has no more bytes
    long fail(const std::string& why);
    std::function<size_t(uint8_t*, size_t)> source_;
    std::vector<uint8_t> in_;      // compressed bytes from file offset in_base_ on
    uint64_t in_base_ = 0, bit_ = 0;   // ... and the next bit to read (relative to in_base_)
    bool in_eof_ = false, in_stream_ = false, done_ = false, bad_ = false;
    uint32_t level_ = 0, combined_ = 0, streams_ = 0;
    std::vector<uint32_t> tt_;   // the inverse BWT's links
    std::vector<uint8_t> ll_;    // the BWT string
    std::vector<uint8_t> out_;
    size_t out_pos_ = 0;
    bz2::Tables* tables_;
    uint32_t crc_tab_[256];
    std::string err_;
};

}  // namespace slimm
