// The lzip format (`lzip`, `plzip`, `tarlz`; the lzip manual's "File format"): the part both the host reader (host/lzip.cpp)
// and the device decoder (lzip_decode.hip) run, the same source for both.  A file is members back to back; a member is
//   header   4C 5A 49 50 ("LZIP"), the version (01; version 0 and any other are refused in words), a dictionary-size byte DS:
//            size = 2^(DS & 31) - (2^(DS & 31) / 16) * (DS >> 5), legal from 4 KiB to 512 MiB
//   stream   one raw LZMA stream with lc = 3, lp = 0, pb = 2, always: fresh state, the probabilities at 1024, an empty
//            dictionary, a first range-coder byte of 0.  It ends with the End Of Stream marker, a match (not a rep) of distance
//            0xFFFFFFFF and length 2 (length 3 is lzlib's sync-flush marker: refused in words, as any other length is), behind
//            which the range coder is normalised once and stands exactly at the trailer's first byte with code == 0
//   trailer  20 bytes, little endian: the CRC32 of the member's text, data_size (u64), member_size (u64: header, stream and
//            trailer)
// The bit-level decoder is xz_stream.h's (Rc, Lzma, the probability layout, lzma_run): lzma_member below is its marked end.
// The decoder is total: every read of input is bounded by the member's stated size (behind the stream, zeros are read and the
// member is refused), every write by its stated data_size, whatever the stream says.  The legacy `.lzma` format is not this.
#pragma once
#include <stdint.h>

#include "xz_stream.h"

namespace slimm {
namespace lzip {

constexpr uint32_t kHeaderBytes = 6, kTrailerBytes = 20;
constexpr uint32_t kMemberMin = kHeaderBytes + 5u + kTrailerBytes;   // (the range coder's five bytes at least)
constexpr uint32_t kDictMin = 1u << 12, kDictMax = 1u << 29;
constexpr uint32_t kLc = 3, kLp = 0, kPb = 2;
constexpr uint32_t kProbs = xz::kLiteral + (xz::kLitSize << (kLc + kLp));   // xz::n_probs(kLc, kLp): 7990 of them, 15 980 bytes

enum Status : uint32_t {
    kOk = 0,
    kRanOut,
    kTrailing,
    kNoMember,
    kVersion0,
    kBadVersion,
    kBadDictSize,
    kBadRangeInit,
    kBadDistance,
    kMatchOverEnd,
    kMarkerEarly,
    kPastEnd,
    kSyncFlush,
    kMarkerLength,
    kStreamEnd,
    kBadRangeEnd,
    kBadCrc,
    kOverrun,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "trailing data behind the last lzip member",
                                                "bytes that start no lzip member",
                                                "lzip version 0 (a member without member_size) is not read",
                                                "an lzip version other than 1",
                                                "a dictionary size below 4 KiB or above 512 MiB",
                                                "a range coder that does not start with a zero byte",
                                                "a distance beyond the member's start or dictionary",
                                                "a match that runs over the member's data_size",
                                                "an end marker in front of the member's data_size",
                                                "text that goes on behind the member's data_size",
                                                "a sync-flush marker (length 3) inside a member",
                                                "an end marker of a length other than 2",
                                                "an LZMA stream that does not end at the member's trailer",
                                                "a range coder that does not end at zero",
                                                "CRC32 mismatch",
                                                "a member that does not lie in the bytes at hand"};
    return s < kStatusCount ? t[s] : "unknown error";
}

SLIMM_XZ_HD inline bool is_magic(const uint8_t* p) { return p[0] == 'L' && p[1] == 'Z' && p[2] == 'I' && p[3] == 'P'; }
// are p[0, n) (n < 4) the first bytes of the magic?  (a file that ends inside it is truncated, not garbage)
SLIMM_XZ_HD inline bool magic_prefix(const uint8_t* p, uint64_t n) {
    const uint8_t m[4] = {'L', 'Z', 'I', 'P'};
    for (uint64_t i = 0; i < n && i < 4u; ++i)
        if (p[i] != m[i]) return false;
    return true;
}
// the DS byte's size (0: not a legal one)
SLIMM_XZ_HD inline uint32_t dict_size_of(uint8_t ds) {
    const uint32_t bits = ds & 31u;
    if (bits < 12u || bits > 29u) return 0;
    const uint32_t size = (1u << bits) - ((1u << bits) / 16u) * (ds >> 5);
    return size < kDictMin || size > kDictMax ? 0u : size;
}
// the six bytes of a header
SLIMM_XZ_HD inline uint32_t member_header(const uint8_t* p, uint32_t* dict_size) {
    if (!is_magic(p)) return kNoMember;
    if (p[4] == 0) return kVersion0;
    if (p[4] != 1u) return kBadVersion;
    *dict_size = dict_size_of(p[5]);
    return *dict_size ? kOk : kBadDictSize;
}

struct Trailer {
    uint32_t crc;
    uint64_t data_size, member_size;
};
SLIMM_XZ_HD inline Trailer member_trailer(const uint8_t* p) { return Trailer{xz::le32(p), xz::le64(p + 4), xz::le64(p + 12)}; }

// Can a stream of `stream_bytes` hold that much text?  A rep match of 273 bytes takes 14 binary decisions of log2(2048 / 2017)
// bits at the least, 0.31 bits: under 7100 bytes of text per byte of stream.  What states more would meet its marker early, and
// is refused as that before memory is asked for
SLIMM_XZ_HD inline bool text_fits_stream(uint64_t data_size, uint64_t stream_bytes) { return data_size <= stream_bytes * 8192u; }

// xz_stream.h's verdict on a run in this format's words
SLIMM_XZ_HD inline uint32_t from_lzma(uint32_t st) {
    switch (st) {
        case xz::kOk: return kOk;
        case xz::kBadRangeInit: return kBadRangeInit;
        case xz::kBadDistance: return kBadDistance;
        case xz::kMatchOverEnd: return kMatchOverEnd;
        case xz::kMarkerEarly: return kMarkerEarly;
        case xz::kPastEnd: return kPastEnd;
        case xz::kSyncFlush: return kSyncFlush;
        case xz::kMarkerLength: return kMarkerLength;
        case xz::kBadRangeEnd: return kBadRangeEnd;
        default: return kStreamEnd;   // (kChunkEnd: the stream ran off its bytes, or stopped in front of the trailer)
    }
}

// One member's stream p[at, end) -- behind its header, in front of its trailer -- decoded to out[0, data_size), which is its
// own dictionary: `probs` holds kProbs probabilities, all at xz::kProbInit
SLIMM_XZ_HD inline uint32_t lzma_member(const uint8_t* p, uint64_t at, uint64_t end, uint16_t* probs, uint8_t* out, uint32_t data_size, uint32_t dict_size,
                                        xz::Tally& t) {
    xz::Lzma s{};
    s.reset_state();
    s.lc = kLc, s.lp = kLp, s.pb = kPb;
    xz::Rc rc;
    uint32_t st = rc.init(p, at, end);
    if (st == xz::kOk) st = xz::lzma_run<true>(rc, s, probs, out, data_size, 0, dict_size, t);
    return from_lzma(st);
}

// (the device decoder describes a member by an xz::Block, whose check is CRC32: `at` its stream's first byte, `end` and
// `check_at` its trailer's -- so the check kernels of xz_decode.hip serve both)

}  // namespace lzip
}  // namespace slimm
