// The header of a BGZF block, parsed at a known start: the one place the host code -- the command's reader
// (host/alignment_file.cpp) and the library's descriptor walk (bgzf_inflate.hip) -- reads it from.  Written from the SAM
// specification, section 4.1:
//   block   1f 8b 08 04 MTIME(4) XFL OS XLEN(2), XLEN bytes of subfields SI1 SI2 SLEN(2) + SLEN bytes -- one of them "BC", SLEN 2,
//           BSIZE = the whole block's bytes - 1 --, the deflate data, CRC32 of the text, ISIZE = its length (64 KiB at the most)
// Plain host C++ without allocation: g++ and hipcc compile it alike, and the walk inlines into its callers' loops.  What a
// status means to a caller -- which words it prints, whether a short tail waits for more bytes or is a truncated file --
// stays with the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace slimm {
namespace bgzf {

constexpr size_t kFixedHeader = 12;   // up to and with XLEN
constexpr size_t kMinHeader = 18;     // ... and a BC subfield, the least a header takes
constexpr uint32_t kMaxIsize = 65536;

enum Status : uint32_t {
    kOk,
    kMore,       // the bytes at hand end inside the block: nothing is wrong with those that are there
    kNotBgzf,    // no gzip member with an extra field (magic, CM = 8, FLG.FEXTRA)
    kNoBc,       // no BC subfield of two bytes in the extra field
    kBadSize,    // BSIZE + 1 does not even hold the header and the trailer
    kTooLarge,   // ISIZE beyond 64 KiB
};

struct Header {
    uint32_t xlen;    // the extra field's bytes (known from the first status that is not kNotBgzf, given kFixedHeader bytes)
    uint32_t total;   // the block's bytes, BSIZE + 1
    uint32_t csize;   // the deflate data's bytes, at p + 12 + xlen
    uint32_t isize, crc;
};

inline uint32_t le16(const uint8_t* p) { return p[0] | (static_cast<uint32_t>(p[1]) << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// The block that starts at p, of which `avail` bytes are at hand; no byte at or beyond p + avail is read.  kOk: the whole
// block is there and *h is filled.
inline Status block_at(const uint8_t* p, size_t avail, Header* h) {
    if (avail < kFixedHeader) return kMore;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return kNotBgzf;
    const uint32_t xlen = h->xlen = le16(p + 10);
    if (avail < kFixedHeader + xlen) return kMore;
    uint32_t total = 0;
    for (uint32_t o = 0; o + 4 <= xlen;) {
        const uint8_t* x = p + kFixedHeader + o;
        const uint32_t slen = le16(x + 2);
        if (x[0] == 'B' && x[1] == 'C' && slen == 2 && o + 6 <= xlen) total = le16(x + 4) + 1u;
        o += 4 + slen;
    }
    if (!total) return kNoBc;
    if (total < kFixedHeader + xlen + 8) return kBadSize;
    if (avail < total) return kMore;
    h->total = total;
    h->csize = total - static_cast<uint32_t>(kFixedHeader) - xlen - 8u;
    h->crc = le32(p + total - 8);
    h->isize = le32(p + total - 4);
    return h->isize > kMaxIsize ? kTooLarge : kOk;
}

// The empty block that ends a file: a fixed-code deflate block that holds its end-of-block code only.  It has nothing to
// inflate; any other payload under an ISIZE of 0 is inflated all the same, and must give no byte and the CRC of none.
inline bool is_eof_block(const uint8_t* payload, size_t csize, uint32_t isize, uint32_t crc) {
    return isize == 0 && csize == 2 && payload[0] == 0x03 && payload[1] == 0x00 && crc == 0;
}

}  // namespace bgzf
}  // namespace slimm
