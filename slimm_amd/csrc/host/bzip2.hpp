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
#include "text_reader.hpp"

namespace slimm {

// error(): "block at byte N: <cause>", "truncated at byte N", ...
class Bzip2Reader : public TextReader {
public:
    explicit Bzip2Reader(Source source);
    ~Bzip2Reader() override;

private:
    bool next_text() override;   // the next block's text, in place of the one before
    bool more_input();   // false: the file has no more bytes
    long fail(const std::string& why);
    uint64_t bit_ = 0;   // the next bit to read, counted from in_[0] (pos_ follows it only for a refill)
    bool in_stream_ = false;
    uint32_t level_ = 0, combined_ = 0, streams_ = 0;
    std::vector<uint32_t> tt_;   // the inverse BWT's links
    std::vector<uint8_t> ll_;    // the BWT string
    bz2::Tables* tables_;
    uint32_t crc_tab_[256];
};

}  // namespace slimm
