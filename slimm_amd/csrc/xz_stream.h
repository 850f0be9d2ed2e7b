// The .xz container and the LZMA2 filter: the part both the host reader (host/xz.cpp) and the device decoder
// (xz_decode.hip) run, the same source for both.  Written from the format as xz writes it (xz-file-format-1.1.0, the LZMA2
// description of XZ Embedded and the LZMA SDK's decoder):
//   stream   header FD 37 7A 58 5A 00, two flag bytes (00, then the check kind in the low nibble), their CRC32; blocks; the
//            index; a footer of CRC32, backward size ((v + 1) * 4 = the index's bytes), the flags again, "YZ".  Streams may
//            follow each other, with multiples of four zero bytes (stream padding) between and behind them
//   block    header: a size byte ((v + 1) * 4 bytes in all), flags (filters - 1 in 2 bits, 4 reserved bits, compressed size
//            stated, uncompressed size stated), the sizes as multibyte integers, the filters {id, bytes of properties, the
//            properties}, zero padding, CRC32; the filter chain's data; zero padding to a multiple of four; the check: none
//            (0 bytes), CRC32 (4), CRC64 (8) or SHA-256 (32) of the block's text
//   index    00, the number of records, {unpadded size = header + data + check, uncompressed size} per block as multibyte
//            integers, zero padding to a multiple of four, CRC32
//   LZMA2    chunks: control 00 ends the data; 01 / 02 an uncompressed chunk (01 resets the dictionary): size - 1 in 2
//            bytes, the bytes; 80..FF an LZMA chunk: bits 0-4 are bits 16-20 of (uncompressed size - 1), then its low 2
//            bytes, (compressed size - 1) in 2 bytes, and by bits 5-6 what is reset first: 0 nothing, 1 the state, 2 the
//            state with a new properties byte (lc + 9 * (lp + 5 * pb), lc + lp <= 4), 3 that and the dictionary
//   LZMA     a range coder (32-bit range, 11-bit adaptive probabilities) over: is_match, is_rep, is_rep0, is_rep0_long,
//            is_rep1, is_rep2 by the 12-state machine; literals in a bit tree chosen by position and previous byte, after a
//            match coded against the byte at the last distance; lengths 2..273 (low, mid, high); a match's distance as a
//            position slot by length, then context-coded, direct and four aligned bits; the four last distances
// A block starts with an empty dictionary and fresh state, and every chunk states both of its sizes: the chunk chain is
// walked from header to header without decoding a bit, and a block is decoded by itself.  The dictionary is the block's own
// text in front of the byte being written: its stated size only bounds the distances.
// The decoder is total: every read of input is bounded by the chunk's stated compressed size (behind it, zeros are read
// and the chunk is refused), every write by its stated uncompressed size, every probability index by construction.
// SHA-256 is NOT verified, by the host reader or the device decoder: such a block is decoded, and counted as unverified.
#pragma once
#include <stdint.h>

#include "deflate_stream.h"

#if defined(__host__) && defined(__device__)
#define SLIMM_XZ_HD __host__ __device__
#else
#define SLIMM_XZ_HD
#endif

namespace slimm {
namespace xz {

constexpr uint32_t kHeaderBytes = 12;            // a stream header, and a footer
constexpr uint32_t kFilterLzma2 = 0x21;
enum Check : uint32_t { kCheckNone = 0, kCheckCrc32 = 1, kCheckCrc64 = 4, kCheckSha256 = 10 };

enum Status : uint32_t {
    kOk = 0,
    kRanOut,
    kTrailing,
    kBadHeaderCrc,
    kBadFlags,
    kBadCheckKind,
    kBadBlockHeader,
    kBadBlockCrc,
    kBadVli,
    kBadFilter,
    kBadDictionary,
    kBadControl,
    kNoDictReset,
    kNoProps,
    kNoStateReset,
    kBadProps,
    kBadRangeInit,
    kBadDistance,
    kMatchOverEnd,
    kChunkEnd,
    kBadRangeEnd,
    kEndMarker,
    kOverrun,
    kBadBlockSizes,
    kBadBlockPadding,
    kBadCheck,
    kBadIndex,
    kBadIndexCrc,
    kIndexMismatch,
    kBadFooter,
    kBadFooterCrc,
    kBadPadding,
    kMarkerEarly,
    kMarkerLength,
    kSyncFlush,
    kPastEnd,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "bytes behind the last stream that are neither padding nor a stream",
                                                "header CRC32 mismatch",
                                                "reserved stream flags are set",
                                                "a check kind other than none, CRC32, CRC64 or SHA-256",
                                                "bad block header",
                                                "block header CRC32 mismatch",
                                                "bad multibyte integer",
                                                "a filter chain other than LZMA2 alone",
                                                "bad LZMA2 dictionary size",
                                                "bad LZMA2 control byte",
                                                "a block's first chunk does not reset the dictionary",
                                                "an LZMA chunk without properties in front of it",
                                                "an LZMA chunk behind an uncompressed chunk does not reset the state",
                                                "bad LZMA properties (lc + lp > 4)",
                                                "a range coder that does not start with a zero byte",
                                                "a distance beyond the block's start or dictionary",
                                                "a match that runs over its chunk's end",
                                                "a chunk that does not end where its compressed size says",
                                                "a range coder that does not end at zero",
                                                "an end marker inside an LZMA2 chunk",
                                                "more text than the chunk headers state",
                                                "block sizes disagree with the block header",
                                                "bad block padding",
                                                "check mismatch",
                                                "bad index",
                                                "index CRC32 mismatch",
                                                "index does not match the blocks",
                                                "bad stream footer",
                                                "footer CRC32 mismatch",
                                                "stream padding that is no multiple of four bytes",
                                                "an end marker in front of the stated size",
                                                "an end marker of a length other than 2",
                                                "a sync-flush marker",
                                                "text that goes on behind the stated size"};
    return s < kStatusCount ? t[s] : "unknown error";
}

SLIMM_XZ_HD inline uint32_t le32(const uint8_t* p) {
    return p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
}
SLIMM_XZ_HD inline uint64_t le64(const uint8_t* p) { return le32(p) | (static_cast<uint64_t>(le32(p + 4)) << 32); }
SLIMM_XZ_HD inline uint32_t be16(const uint8_t* p) { return (static_cast<uint32_t>(p[0]) << 8) | p[1]; }

// ---- the checks.  CRC32: deflate_stream.h (gz::crc_table_entry, crc_mul, crc_x_pow8).  CRC64: ECMA-182, reflected, the
// same three for 64 bits.  A register is stepped from any start r over n bytes d as r * x^(8 n) + reg(0, d) (mod P), which is
// how pieces of a text, each taken from 0, are folded
constexpr uint64_t kCrc64Poly = 0xC96C5795D7870F42ull;
SLIMM_XZ_HD inline uint64_t crc64_table_entry(uint32_t i) {
    uint64_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrc64Poly : c >> 1;
    return c;
}
SLIMM_XZ_HD inline uint64_t crc64_mul(uint64_t a, uint64_t b) {
    uint64_t p = 0;
    for (uint64_t m = 1ull << 63; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrc64Poly : b >> 1;
    }
    return p;
}
SLIMM_XZ_HD inline uint64_t crc64_x_pow8(uint64_t n_bytes) {   // x^(8 n) mod P
    uint64_t p = 1ull << 63, sq = 1ull << 55;   // sq = x^8
    for (; n_bytes; n_bytes >>= 1) {
        if (n_bytes & 1u) p = crc64_mul(sq, p);
        sq = crc64_mul(sq, sq);
    }
    return p;
}
// CRC32 of a few bytes (the headers), without a table
SLIMM_XZ_HD inline uint32_t crc32_small(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) c = gz::crc_table_entry((c ^ p[i]) & 0xffu) ^ (c >> 8);
    return ~c;
}
SLIMM_XZ_HD inline uint32_t check_bytes(uint32_t kind) { return kind == kCheckCrc32 ? 4u : kind == kCheckCrc64 ? 8u : kind == kCheckSha256 ? 32u : 0u; }

// ---- the container
// A multibyte integer at p[*pos] (at most 9 bytes, 63 bits): kRanOut when p[0, avail) ends inside it
SLIMM_XZ_HD inline uint32_t vli(const uint8_t* p, uint64_t avail, uint64_t* pos, uint64_t* v) {
    uint64_t out = 0;
    for (uint32_t i = 0; i < 9u; ++i) {
        if (*pos >= avail) return kRanOut;
        const uint8_t b = p[(*pos)++];
        out |= static_cast<uint64_t>(b & 0x7fu) << (7u * i);
        if (!(b & 0x80u)) {
            if (b == 0 && i > 0) return kBadVli;
            *v = out;
            return kOk;
        }
    }
    return kBadVli;
}

SLIMM_XZ_HD inline bool is_magic(const uint8_t* p) { return p[0] == 0xfd && p[1] == '7' && p[2] == 'z' && p[3] == 'X' && p[4] == 'Z' && p[5] == 0; }
// are p[0, n) (n < 6) the first bytes of the magic?  (a file that ends inside it is truncated, not garbage)
SLIMM_XZ_HD inline bool magic_prefix(const uint8_t* p, uint64_t n) {
    const uint8_t m[6] = {0xfd, '7', 'z', 'X', 'Z', 0};
    for (uint64_t i = 0; i < n && i < 6u; ++i)
        if (p[i] != m[i]) return false;
    return true;
}
// the 12 bytes of a stream header (the magic is there: is_magic) -> the check kind
SLIMM_XZ_HD inline uint32_t stream_header(const uint8_t* p, uint32_t* check) {
    if (crc32_small(p + 6, 2) != le32(p + 8)) return kBadHeaderCrc;
    if (p[6] != 0 || (p[7] & 0xf0u)) return kBadFlags;
    *check = p[7];
    if (*check != kCheckNone && *check != kCheckCrc32 && *check != kCheckCrc64 && *check != kCheckSha256) return kBadCheckKind;
    return kOk;
}
// the 12 bytes of a footer -> the index's bytes
SLIMM_XZ_HD inline uint32_t stream_footer(const uint8_t* p, uint32_t check, uint64_t* index_bytes) {
    if (p[10] != 'Y' || p[11] != 'Z') return kBadFooter;
    if (crc32_small(p + 4, 6) != le32(p)) return kBadFooterCrc;
    if (p[8] != 0 || p[9] != check) return kBadFooter;
    *index_bytes = (static_cast<uint64_t>(le32(p + 4)) + 1u) * 4u;
    return kOk;
}

struct BlockHeader {
    uint32_t bytes;            // the header's
    uint32_t dict_size;
    uint32_t filter_id;        // kBadFilter: the first filter that is not LZMA2
    bool has_compressed, has_uncompressed;
    uint64_t compressed, uncompressed;
};
// A block header at p[0, avail), p[0] != 0 (that is the index)
SLIMM_XZ_HD inline uint32_t block_header(const uint8_t* p, uint64_t avail, BlockHeader& h) {
    if (avail < 1u) return kRanOut;
    h.bytes = (static_cast<uint32_t>(p[0]) + 1u) * 4u;
    if (avail < h.bytes) return kRanOut;
    const uint64_t end = h.bytes - 4u;
    if (crc32_small(p, end) != le32(p + end)) return kBadBlockCrc;
    const uint8_t flags = p[1];
    if (flags & 0x3cu) return kBadBlockHeader;
    const uint32_t n_filters = (flags & 3u) + 1u;
    h.has_compressed = flags & 0x40u, h.has_uncompressed = flags & 0x80u;
    h.compressed = h.uncompressed = 0;
    uint64_t pos = 2;
    if (h.has_compressed && vli(p, end, &pos, &h.compressed) != kOk) return kBadBlockHeader;
    if (h.has_compressed && h.compressed == 0) return kBadBlockHeader;
    if (h.has_uncompressed && vli(p, end, &pos, &h.uncompressed) != kOk) return kBadBlockHeader;
    uint32_t status = kOk;
    h.filter_id = kFilterLzma2;
    h.dict_size = 0;
    for (uint32_t f = 0; f < n_filters; ++f) {
        uint64_t id = 0, n_props = 0;
        if (vli(p, end, &pos, &id) != kOk || vli(p, end, &pos, &n_props) != kOk || n_props > end - pos) return kBadBlockHeader;
        if (id != kFilterLzma2) {
            if (status == kOk) h.filter_id = static_cast<uint32_t>(id < 0xffffffffu ? id : 0xffffffffu);
            status = kBadFilter;
        } else {
            if (n_props != 1u) return kBadBlockHeader;
            const uint32_t d = p[pos];
            if (d > 40u) return kBadDictionary;
            h.dict_size = d == 40u ? 0xffffffffu : (2u | (d & 1u)) << (d / 2u + 11u);
        }
        pos += n_props;
    }
    for (; pos < end; ++pos)
        if (p[pos]) return kBadBlockHeader;
    if (status == kOk && n_filters != 1u) status = kBadFilter;   // (LZMA2 twice: filter_id says LZMA2)
    return status;
}

// The index at p[0, avail) (p[0] == 0): its bytes in all, the number of its records and where the first of them starts; the
// records' integers, the padding and the CRC32 are checked.  kRanOut: p[0, avail) ends inside it
SLIMM_XZ_HD inline uint32_t index_extent(const uint8_t* p, uint64_t avail, uint64_t* count, uint64_t* first_record, uint64_t* bytes) {
    uint64_t pos = 1, v = 0;
    uint32_t st = vli(p, avail, &pos, count);
    if (st != kOk) return st == kRanOut ? kRanOut : kBadIndex;
    *first_record = pos;
    for (uint64_t i = 0; i < *count; ++i)
        for (uint32_t k = 0; k < 2u; ++k) {
            st = vli(p, avail, &pos, &v);
            if (st != kOk) return st == kRanOut ? kRanOut : kBadIndex;
        }
    for (; pos & 3u; ++pos) {
        if (pos >= avail) return kRanOut;
        if (p[pos]) return kBadIndex;
    }
    if (avail - pos < 4u) return kRanOut;
    if (crc32_small(p, pos) != le32(p + pos)) return kBadIndexCrc;
    *bytes = pos + 4u;
    return kOk;
}
// the next record of an index that index_extent has taken
SLIMM_XZ_HD inline void index_record(const uint8_t* p, uint64_t avail, uint64_t* pos, uint64_t* unpadded, uint64_t* uncompressed) {
    (void)vli(p, avail, pos, unpadded);
    (void)vli(p, avail, pos, uncompressed);
}

// ---- LZMA2 chunks
struct Chunk {
    uint32_t control;    // 0: the end marker
    uint32_t header;     // the header's bytes
    uint32_t usize, csize;   // text bytes; the bytes behind the header (an uncompressed chunk: = usize)
    bool lzma, dict_reset, state_reset, new_props;
    uint32_t lc, lp, pb;
    uint8_t props;
};
// what the chunks so far demand of the next one
struct Rules {
    bool need_dict = true, need_props = true, need_state = true;
};
// The chunk header at p[0, avail) against the rules, which move on; kRanOut: the bytes end inside it
SLIMM_XZ_HD inline uint32_t chunk_header(const uint8_t* p, uint64_t avail, Rules& r, Chunk& c) {
    if (avail < 1u) return kRanOut;
    c.control = p[0];
    c.header = 1, c.usize = c.csize = 0;
    c.lzma = c.dict_reset = c.state_reset = c.new_props = false;
    c.lc = c.lp = c.pb = 0, c.props = 0;
    if (c.control == 0) return kOk;
    if (c.control >= 0x80u) {
        c.lzma = true;
        const uint32_t reset = (c.control >> 5) & 3u;
        c.header = reset >= 2u ? 6u : 5u;
        if (avail < c.header) return kRanOut;
        c.usize = (((c.control & 0x1fu) << 16) | be16(p + 1)) + 1u;
        c.csize = be16(p + 3) + 1u;
        c.dict_reset = reset == 3u, c.new_props = reset >= 2u, c.state_reset = reset >= 1u;
        if (r.need_dict && !c.dict_reset) return kNoDictReset;
        if (r.need_props && !c.new_props) return kNoProps;
        if (r.need_state && !c.state_reset) return kNoStateReset;
        if (c.new_props) {
            uint32_t d = c.props = p[5];
            if (d > (4u * 5u + 4u) * 9u + 8u) return kBadProps;
            c.lc = d % 9u, d /= 9u;
            c.lp = d % 5u, c.pb = d / 5u;
            if (c.lc + c.lp > 4u) return kBadProps;
        }
        r.need_dict = r.need_props = r.need_state = false;
        return kOk;
    }
    if (c.control > 2u) return kBadControl;
    c.header = 3;
    if (avail < c.header) return kRanOut;
    c.usize = c.csize = be16(p + 1) + 1u;
    c.dict_reset = c.control == 1u;
    if (r.need_dict && !c.dict_reset) return kNoDictReset;
    if (c.dict_reset) r.need_props = true;   // (a dictionary reset: the next LZMA chunk sets its properties anew)
    r.need_dict = false;
    r.need_state = true;
    return kOk;
}

// ---- the LZMA decoder
// the probabilities, 11 bits each in 16: 1846 whatever the properties, then 0x300 per literal context.  A bit tree of n
// bits takes 1 << n of them and leaves the first unused
constexpr uint32_t kPosStatesMax = 16;
constexpr uint32_t kIsMatch = 0, kIsRep = 192, kIsRepG0 = 204, kIsRepG1 = 216, kIsRepG2 = 228, kIsRep0Long = 240, kPosSlot = 432, kSpecPos = 688, kAlign = 802,
                   kMatchLen = 818, kRepLen = 1332, kLiteral = 1846;
constexpr uint32_t kLitSize = 0x300, kProbsMax = kLiteral + (kLitSize << 4);
constexpr uint16_t kProbInit = 1024;
SLIMM_XZ_HD inline uint32_t n_probs(uint32_t lc, uint32_t lp) { return kLiteral + (kLitSize << (lc + lp)); }

struct Lzma {
    uint32_t state, rep[4];
    uint32_t lc, lp, pb;
    SLIMM_XZ_HD void reset_state() { state = 0, rep[0] = rep[1] = rep[2] = rep[3] = 0; }
};
// what a block's chunks did (the device's counters, the tests' census)
struct Tally {
    uint64_t match_bytes;
    uint32_t max_dist;
};

// The range decoder over p[pos, end): behind `end` it reads zeros and remembers that it did
struct Rc {
    const uint8_t* p;
    uint64_t pos, end;
    uint32_t range, code, over;
    SLIMM_XZ_HD uint32_t init(const uint8_t* bytes, uint64_t at, uint64_t end_) {
        p = bytes, pos = at, end = end_, range = 0xffffffffu, code = 0, over = 0;
        if (end - at < 5u) return kChunkEnd;
        if (p[pos] != 0) return kBadRangeInit;
        ++pos;
        for (uint32_t i = 0; i < 4u; ++i) code = (code << 8) | p[pos++];
        return kOk;
    }
    SLIMM_XZ_HD void normalize() {
        if (range < (1u << 24)) {
            range <<= 8;
            uint32_t b = 0;
            if (pos < end) b = p[pos++];
            else
                over = 1;
            code = (code << 8) | b;
        }
    }
    SLIMM_XZ_HD uint32_t bit(uint16_t& prob) {
        normalize();
        const uint32_t pr = prob, bound = (range >> 11) * pr;
        if (code < bound) {
            range = bound;
            prob = static_cast<uint16_t>(pr + ((2048u - pr) >> 5));
            return 0;
        }
        range -= bound, code -= bound;
        prob = static_cast<uint16_t>(pr - (pr >> 5));
        return 1;
    }
    // n bits through the tree at probs[1, 1 << n): the symbol without its leading one
    SLIMM_XZ_HD uint32_t tree(uint16_t* probs, uint32_t n) {
        uint32_t m = 1;
        for (uint32_t i = 0; i < n; ++i) m = (m << 1) | bit(probs[m]);
        return m - (1u << n);
    }
    SLIMM_XZ_HD uint32_t tree_reverse(uint16_t* probs, uint32_t n) {
        uint32_t m = 1, v = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t b = bit(probs[m]);
            m = (m << 1) | b;
            v |= b << i;
        }
        return v;
    }
    SLIMM_XZ_HD uint32_t direct(uint32_t n) {
        uint32_t v = 0;
        for (uint32_t i = 0; i < n; ++i) {
            normalize();
            range >>= 1;
            code -= range;
            const uint32_t mask = 0u - (code >> 31);
            code += range & mask;
            v = (v << 1) + (mask + 1u);
        }
        return v;
    }
};

SLIMM_XZ_HD inline uint32_t lzma_len(Rc& rc, uint16_t* l, uint32_t pos_state) {
    if (!rc.bit(l[0])) return 2u + rc.tree(l + 2u + pos_state * 8u, 3);
    if (!rc.bit(l[1])) return 10u + rc.tree(l + 130u + pos_state * 8u, 3);
    return 18u + rc.tree(l + 258u, 8);
}

// The LZMA symbols of one run of `usize` text bytes to out[0, usize), of which out[-since, 0) are the `since` bytes written
// since the last dictionary reset (the dictionary: a distance reaches min(since + written, dict_size) back at most); the
// compressed bytes are rc's, which has been started (Rc::init).  The one body of the two ways a run ends:
//   an LZMA2 chunk (kMarked = false)   after exactly usize bytes; an end marker is kEndMarker
//   an lzip member (kMarked = true)    with the end marker -- a match, not a rep, of distance 0xFFFFFFFF and length 2 -- behind
//                                      exactly usize bytes: earlier kMarkerEarly, a literal or a short rep there kPastEnd, a
//                                      match there kMatchOverEnd; length 3 is kSyncFlush, any other kMarkerLength
// Behind either the coder is normalised once and stands at rc.end with code 0.  No byte is written at or behind out[usize]
template <bool kMarked>
SLIMM_XZ_HD inline uint32_t lzma_run(Rc& rc, Lzma& s, uint16_t* probs, uint8_t* out, uint32_t usize, uint64_t since, uint32_t dict_size, Tally& t) {
    const uint32_t pos_mask = (1u << s.pb) - 1u, lp_mask = (1u << s.lp) - 1u;
    uint32_t n = 0;
    while (kMarked || n < usize) {
        if (rc.over) return kChunkEnd;
        const uint64_t at = since + n;
        const uint32_t pos_state = static_cast<uint32_t>(at) & pos_mask;
        const int64_t o = static_cast<int64_t>(n);
        if (!rc.bit(probs[kIsMatch + s.state * kPosStatesMax + pos_state])) {
            if (kMarked && n == usize) return kPastEnd;
            const uint32_t prev = at ? out[o - 1] : 0u;
            uint16_t* lit = probs + kLiteral + kLitSize * (((static_cast<uint32_t>(at) & lp_mask) << s.lc) + (prev >> (8u - s.lc)));
            uint32_t sym = 1;
            if (s.state < 7u) {
                while (sym < 0x100u) sym = (sym << 1) | rc.bit(lit[sym]);
            } else {
                // (the state says a match came last: its distance was checked when it was used -- a guard all the same)
                if (s.rep[0] >= at) return kBadDistance;
                uint32_t match = out[o - static_cast<int64_t>(s.rep[0]) - 1], offs = 0x100u;
                while (sym < 0x100u) {
                    match <<= 1;
                    const uint32_t mb = match & offs, b = rc.bit(lit[offs + mb + sym]);
                    sym = (sym << 1) | b;
                    offs &= b ? mb : ~mb;
                }
            }
            out[o] = static_cast<uint8_t>(sym);
            ++n;
            s.state = s.state < 4u ? 0u : s.state < 10u ? s.state - 3u : s.state - 6u;
            continue;
        }
        uint32_t len;
        if (!rc.bit(probs[kIsRep + s.state])) {
            s.rep[3] = s.rep[2], s.rep[2] = s.rep[1], s.rep[1] = s.rep[0];
            len = lzma_len(rc, probs + kMatchLen, pos_state);
            s.state = s.state < 7u ? 7u : 10u;
            const uint32_t slot = rc.tree(probs + kPosSlot + (len < 6u ? len - 2u : 3u) * 64u, 6);
            uint32_t d = slot;
            if (slot >= 4u) {
                const uint32_t limit = (slot >> 1) - 1u;
                d = 2u | (slot & 1u);
                if (slot < 14u) {
                    d <<= limit;
                    d += rc.tree_reverse(probs + kSpecPos + d - slot - 1u, limit);
                } else {
                    d = (d << (limit - 4u)) + rc.direct(limit - 4u);
                    d = (d << 4) + rc.tree_reverse(probs + kAlign, 4);
                }
            }
            if (d == 0xffffffffu) {
                if (!kMarked) return kEndMarker;
                if (len != 2u) return len == 3u ? kSyncFlush : kMarkerLength;
                if (n < usize) return kMarkerEarly;
                break;
            }
            s.rep[0] = d;
        } else {
            if (!rc.bit(probs[kIsRepG0 + s.state])) {
                if (!rc.bit(probs[kIsRep0Long + s.state * kPosStatesMax + pos_state])) {
                    if (kMarked && n == usize) return kPastEnd;
                    if (s.rep[0] >= at || s.rep[0] >= dict_size) return kBadDistance;
                    out[o] = out[o - static_cast<int64_t>(s.rep[0]) - 1];
                    ++n;
                    ++t.match_bytes;
                    if (s.rep[0] + 1u > t.max_dist) t.max_dist = s.rep[0] + 1u;
                    s.state = s.state < 7u ? 9u : 11u;
                    continue;
                }
            } else {
                uint32_t d;
                if (!rc.bit(probs[kIsRepG1 + s.state])) d = s.rep[1];
                else {
                    if (!rc.bit(probs[kIsRepG2 + s.state])) d = s.rep[2];
                    else {
                        d = s.rep[3];
                        s.rep[3] = s.rep[2];
                    }
                    s.rep[2] = s.rep[1];
                }
                s.rep[1] = s.rep[0];
                s.rep[0] = d;
            }
            len = lzma_len(rc, probs + kRepLen, pos_state);
            s.state = s.state < 7u ? 8u : 11u;
        }
        if (s.rep[0] >= at || s.rep[0] >= dict_size) return kBadDistance;
        if (len > usize - n) return kMatchOverEnd;
        const int64_t back = static_cast<int64_t>(s.rep[0]) + 1;
        // (eight bytes a trip where the copy does not read what it has just written: the loads go out together, which is
        // what a lane that waits out every load's latency gains from)
        uint32_t k = 0;
        if (back >= 8) {
            for (; k + 8u <= len; k += 8u) {
                uint8_t v[8];
                for (uint32_t j = 0; j < 8u; ++j) v[j] = out[o + k + j - back];
                for (uint32_t j = 0; j < 8u; ++j) out[o + k + j] = v[j];
            }
        }
        for (; k < len; ++k) out[o + k] = out[o + k - back];
        n += len;
        t.match_bytes += len;
        if (s.rep[0] + 1u > t.max_dist) t.max_dist = s.rep[0] + 1u;
    }
    rc.normalize();
    if (rc.over || rc.pos != rc.end) return kChunkEnd;
    if (rc.code != 0) return kBadRangeEnd;
    return kOk;
}
// One LZMA chunk of LZMA2: the state and the probabilities go on from chunk to chunk
SLIMM_XZ_HD inline uint32_t lzma_chunk(Rc& rc, Lzma& s, uint16_t* probs, uint8_t* out, uint32_t usize, uint64_t since, uint32_t dict_size, Tally& t) {
    return lzma_run<false>(rc, s, probs, out, usize, since, dict_size, t);
}

// ---- a block for the device decoder (xz_decode.hip): where it lies in the round's bytes and text, and what decoding found
struct Block {
    uint64_t at, end;            // its first chunk's byte; the byte behind its end marker
    uint64_t text_at, text_len;  // in the round's text
    uint64_t check_at;           // its check field
    uint64_t last_mul;           // x^(8 * the bytes of its last piece), for its check kind
    uint64_t crc;                // the check's register over the text, from 0
    uint64_t match_bytes;
    uint32_t dict_size, check, piece0, status;
    uint32_t lzma_chunks, raw_chunks, state_resets, prop_changes, odd_props, max_dist;
};

// a piece of a block's text (gz::kPiece bytes): its check register from 0
struct Piece {
    uint64_t reg, unused;
};

}  // namespace xz
}  // namespace slimm
