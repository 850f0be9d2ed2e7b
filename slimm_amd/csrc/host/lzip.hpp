// lzip on the host: one serial decoder for the SAM header of an lzip-compressed SAM file, for `--host-decode`,
// `--dump-records` / `--dump-raw` (the reader thread), redirected standard input, the read-length sample, files of few
// members, and the CPU tests.  The format is ../lzip_member.h and the member finder ../lzip_walk.h, the device decoder's own
// sources.  No lzlib and no liblzma: the command does not depend on them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../lzip_walk.h"
#include "text_reader.hpp"

namespace slimm {

// error(): "member at byte N: <cause>", "at byte N: trailing data behind the last lzip member"
class LzipReader : public TextReader {
public:
    // what the file held so far (the tests compare with their own walk; the device decoder counts the same)
    struct Counts {
        uint64_t members = 0, empty_members = 0, crc32_checked = 0, match_bytes = 0, max_dist = 0, max_dict = 0, text = 0;
    };
    explicit LzipReader(Source source) : TextReader(std::move(source)) {}
    const Counts& counts() const { return n_; }

private:
    bool next_text() override;   // the next member that holds text, whole
    bool fail(const std::string& words);
    lzip::Walker walk_;
    std::vector<uint16_t> probs_;
    Counts n_;
};

// A member by the trailers: where it starts, its bytes and its text's
struct LzipIndexMember {
    uint64_t at, member_size, data_size;
};
// A file of `size` bytes seen through read(offset, dst, n) (false: a read error): its members in file order, read from the
// file's end -- a trailer's member_size names the member's start, the trailer in front of it the one before --, every
// member's header held against the format.  Nothing is decoded.  false: the chain does not close on byte 0
bool lzip_read_index(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, std::vector<LzipIndexMember>* members);

}  // namespace slimm
