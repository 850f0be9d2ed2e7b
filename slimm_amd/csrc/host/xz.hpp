// xz on the host: one serial decoder for the SAM header of an xz-compressed SAM file, for `--host-decode`,
// `--verify-grouping`, `--packed-records`, pipes and `--dump-records` / `--dump-raw` (the reader thread), for files of few
// blocks, and for the CPU tests.  The format is ../xz_stream.h, the device decoder's own source; streams back to back, with
// stream padding, are read one after the other.  LZMA2 is the one filter; SHA-256 checks are not verified.  No liblzma:
// the command does not depend on it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../xz_walk.h"
#include "text_reader.hpp"

namespace slimm {

// error(): "block at byte N: <cause>", "index at byte N: <cause>", ...
class XzReader : public TextReader {
public:
    // what the file held so far (the tests compare with their own walk; the device decoder counts the same)
    struct Counts {
        uint64_t streams = 0, blocks = 0, lzma_chunks = 0, raw_chunks = 0, state_resets = 0, prop_changes = 0, odd_props = 0;
        uint64_t check_none = 0, check_crc32 = 0, check_crc64 = 0, sha256_unverified = 0;
        uint64_t match_bytes = 0, max_dist = 0, text = 0, index_records = 0;
    };
    explicit XzReader(Source source) : TextReader(std::move(source)) {}
    const Counts& counts() const { return n_; }

private:
    bool next_text() override;   // the next chunk that holds text, behind the block's text so far (at least its dictionary's worth is kept)
    bool fail(const std::string& words);
    xz::Walker walk_;   // the container: where the reader stands in it, the stream's check kind and records, the block at hand
    uint64_t since_ = 0, crc_ = 0;   // the block's text since its last dictionary reset, its check register
    xz::Lzma lz_{};
    std::vector<uint16_t> probs_;
    Counts n_;
};

// A block by its stream's index: where its header lies in the file, its unpadded size (header, data and check) and its text
struct XzIndexBlock {
    uint64_t at, unpadded, uncompressed;
    uint32_t stream;
};
// A file of `size` bytes seen through read(offset, dst, n) (false: a read error): the blocks of all its streams in file
// order, read from the file's end -- footer, backward size, index, the stream's header, stream padding, the stream in front.
// false: it does not parse that way (nothing is decoded: the blocks themselves are not looked at)
// (layout, where asked for: every stream in file order -- one without blocks too --, its header's first byte, the byte behind
// its footer, its check kind and how many blocks it has)
struct XzIndexStream {
    uint64_t at, end, blocks;
    uint32_t check;
};
bool xz_read_index(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, std::vector<XzIndexBlock>* blocks, uint32_t* streams,
                   std::vector<XzIndexStream>* layout = nullptr);

// Where a file may be cut into byte ranges (split.hip: slimm_host_xz_ranges), by its index or indexes alone.  A legal cut is
// the first byte of a block that is not the first of its stream, the first byte of a stream header -- the cut in front of a
// stream's first block: stream padding stays on the left --, or the file's size; none lies in front of the end of the block
// that holds decoded byte skip - 1.  offsets[0] = 0, offsets[n] = size, offsets[i] the earliest legal cut at or behind member
// i's even share of the bytes behind the first legal one.  false: the index does not parse, or states less text than `skip`
bool xz_plan_ranges(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t skip, uint32_t n, uint64_t* offsets);
// ... the same over an index that xz_read_index has read already (its blocks and its layout)
bool xz_plan_ranges(const std::vector<XzIndexBlock>& blocks, const std::vector<XzIndexStream>& layout, uint64_t size, uint64_t skip, uint32_t n,
                    uint64_t* offsets);
// What a range that starts at `offset` cannot see: the check kind of the stream whose blocks it starts among (from that
// stream's footer) -- or -1, when offset is 0, a stream header's first byte, or no byte of a stream.  false as above
bool xz_check_at(const std::function<bool(uint64_t, uint8_t*, size_t)>& read, uint64_t size, uint64_t offset, int* check);

}  // namespace slimm
