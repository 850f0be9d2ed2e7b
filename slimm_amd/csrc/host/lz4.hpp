// LZ4 on the host: one serial decoder for the SAM header of an lz4-compressed SAM file, for `--host-decode`,
// `--verify-grouping`, `--packed-records`, pipes and `--dump-records` / `--dump-raw` (the reader thread), and for the CPU
// tests.  The format is ../lz4_frame.h, the device decoder's own source, the container ../lz4_walk.h; frames back to back
// are read one after the other, skippable frames passed over.  No liblz4: the command does not depend on it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../lz4_walk.h"
#include "text_reader.hpp"

namespace slimm {

// error(): "block at byte N: <cause>", "frame at byte N: <cause>", ...
class Lz4Reader : public TextReader {
public:
    explicit Lz4Reader(Source source) : TextReader(std::move(source)) {}
    // one compressed block's bytes -> its text behind `text`, whose bytes from `lo` on are what a match may reach (the
    // frame's so far in a linked frame, none in an independent one): the serial use of lz4_frame.h, also what the tests
    // compare the device decoder with
    static uint32_t decode_block(const uint8_t* p, uint32_t size, uint32_t block_max, std::vector<uint8_t>& text, size_t lo);

private:
    bool next_text() override;   // the next block that holds text, behind the frame's text so far (at least its last 64 KiB are kept)
    bool fail(const std::string& where, uint32_t status);
    lz4::Walker walk_;   // the frames and block headers: where the reader stands in them
    uint64_t frame_len_ = 0;
    lz4::Xxh32 xxh_;
};

}  // namespace slimm
