// zstd on the host: one serial decoder for the SAM header of a zstd-compressed SAM file, for `--host-decode`,
// `--verify-grouping`, `--packed-records`, pipes and `--dump-records` / `--dump-raw` (the reader thread), and for the CPU
// tests.  The format is ../zstd_frame.h, the device decoder's own source; frames back to back (pzstd, cat) are read one
// after the other, skippable frames passed over.  No libzstd: the command does not depend on it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../zstd_walk.h"
#include "text_reader.hpp"

namespace slimm {

// error(): "block at byte N: <cause>", "frame at byte N: <cause>", ...
class ZstdReader : public TextReader {
public:
    explicit ZstdReader(Source source) : TextReader(std::move(source)) {}
    // where the reader stands: the file offset behind the last block it decoded (its checksum included), whether a frame
    // goes on there, and that frame's header (the split planner walks on from here: split.hip)
    uint64_t file_pos() const { return in_base_ + pos_; }
    bool in_frame() const { return walk_.stage != zs::Walker::Between; }
    const zs::FrameHeader& frame() const { return walk_.fh; }
    // one compressed block's content -> its text behind `text` (whose bytes from frame_lo on are the frame's so far):
    // the serial use of zstd_frame.h, also what the tests compare the device decoder's stages with
    static uint32_t decode_compressed(const uint8_t* content, uint32_t size, uint32_t block_max, uint64_t window, zs::Entropy& e, uint32_t rep[3],
                                      std::vector<uint8_t>& text, size_t frame_lo);

private:
    bool next_text() override;   // the next block that holds text, behind the frame's text so far (at least its last `window` bytes are kept)
    bool fail(const std::string& where, uint32_t status);
    zs::Walker walk_;   // the frames and block headers: where the reader stands in them
    uint64_t frame_len_ = 0;
    zs::Entropy entropy_;
    uint32_t rep_[3] = {1, 4, 8};
    zs::Xxh64 xxh_;
};

// A file of `size` bytes seen through read(offset, dst, n) (false: a read error): *end = the first byte behind the frame
// that holds decoded byte skip - 1 -- the first place where a file split by byte range may be cut, since the first range
// holds the whole SAM header (0 for skip = 0).  The frames up to there are decoded, the last one's block chain is walked to
// its end.  false: they do not decode, or end in front of decoded byte `skip`
bool zstd_header_end(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t skip, uint64_t* end);

}  // namespace slimm
