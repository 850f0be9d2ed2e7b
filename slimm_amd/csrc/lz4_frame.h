// The LZ4 frame format: the part both the host reader (host/lz4.cpp) and the device decoder (lz4_decode.hip) run, the same
// source for both.  Written from the format as lz4 writes it (lz4_Frame_format.md, lz4_Block_format.md):
//   frame     magic 04 22 4D 18, FLG (version 2 bits = 01, block independence, block checksum, content size, content
//             checksum, reserved, dictionary id), BD (reserved, block maximum 3 bits: 4..7 = 64 KiB, 256 KiB, 1 MiB, 4 MiB,
//             4 reserved bits), a content size of 8 bytes and a dictionary id of 4 where FLG says so, HC = the second byte
//             of XXH32 over FLG .. HC - 1; blocks; the end mark (a block header of 0); the text's XXH32 where FLG says so
//   skippable magic 0x184D2A5?, a 4-byte length, that many bytes (zstd's skippable frame: the two formats share it)
//   legacy    magic 02 21 4C 18 (`lz4 -l`): refused
//   block     4 bytes, little endian: the top bit = stored, the rest its size -- at most the block maximum --; the bytes;
//             their XXH32 where FLG says so
//   compressed block = sequences: a token (literal length nibble, match length nibble), the literal length's extension
//             (nibble 15: bytes added until one is below 255), the literals, a 2-byte offset (0 is invalid), the match
//             length's extension; match length = nibble + 4 + extension.  The last sequence is literals only and ends at
//             the block's last byte.  In a linked frame (`lz4 -BD`) a match reaches up to 65 535 bytes back into the
//             frame's text in front of the block, in an independent frame only into the block's own
// Everything that loops here is counted by a size the headers state; nothing indexes outside what it is given.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__host__) && defined(__device__)
#define SLIMM_LZ4_HD __host__ __device__
#else
#define SLIMM_LZ4_HD
#endif

namespace slimm {
namespace lz4 {

constexpr uint32_t kMagic = 0x184D2204u, kLegacyMagic = 0x184C2102u, kSkippable = 0x184D2A50u;
constexpr uint32_t kHistory = 64u << 10;      // what a linked block may reach back into: the frame's last 64 KiB
constexpr uint32_t kBlockMaxMost = 4u << 20;

enum Status : uint32_t {
    kOk = 0,
    kRanOut,
    kNoFrame,
    kNotLz4,
    kLegacy,
    kBadVersion,
    kReservedBit,
    kDictionary,
    kBadBlockMax,
    kBadHeaderChecksum,
    kBlockTooLarge,
    kBadBlockChecksum,
    kBadContentSize,
    kBadChecksum,
    kZeroOffset,
    kBadOffset,
    kEndsInLength,
    kEndsInLiterals,
    kEndsInOffset,
    kEndsBehindMatch,
    kTextTooLarge,
    kTooManySequences,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "bytes behind the last frame that start no frame",
                                                "no lz4 frame starts here",
                                                "the legacy lz4 format (lz4 -l): not supported",
                                                "a frame version other than 1",
                                                "a reserved bit is set",
                                                "a dictionary is needed: not supported",
                                                "a block maximum below 64 KiB: reserved",
                                                "header checksum mismatch",
                                                "a block larger than its maximum",
                                                "block checksum mismatch",
                                                "content size mismatch",
                                                "content checksum mismatch",
                                                "an offset of 0",
                                                "an offset beyond the frame's start, or beyond the block's in an independent frame",
                                                "a block that ends inside a length",
                                                "a block that ends inside its literals",
                                                "a block that ends inside an offset",
                                                "a block that ends behind a match: its last sequence is literals only",
                                                "a block whose text is larger than its maximum",
                                                "internal error: more sequences than a block's bytes allow"};
    return s < kStatusCount ? t[s] : "unknown error";
}

SLIMM_LZ4_HD inline uint32_t le16(const uint8_t* p) { return p[0] | (static_cast<uint32_t>(p[1]) << 8); }
SLIMM_LZ4_HD inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// ---- XXH32, seed 0 (host): the header's, the blocks' and the content's checksum
struct Xxh32 {
    static constexpr uint32_t P1 = 0x9E3779B1u, P2 = 0x85EBCA77u, P3 = 0xC2B2AE3Du, P4 = 0x27D4EB2Fu, P5 = 0x165667B1u;
    uint32_t v[4] = {P1 + P2, P2, 0u, 0u - P1};
    uint64_t total = 0;
    uint8_t tail[16] = {};
    uint32_t n_tail = 0;
    static uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
    static uint32_t round(uint32_t acc, uint32_t in) { return rotl(acc + in * P2, 13) * P1; }
    void reset() { *this = Xxh32(); }
    void stripe(const uint8_t* p) {
        for (int i = 0; i < 4; ++i) v[i] = round(v[i], le32(p + 4 * i));
    }
    void update(const uint8_t* p, uint64_t n) {
        total += n;
        if (n_tail) {
            const uint64_t take = n < 16u - n_tail ? n : 16u - n_tail;
            memcpy(tail + n_tail, p, take);
            n_tail += static_cast<uint32_t>(take), p += take, n -= take;
            if (n_tail < 16u) return;
            stripe(tail);
            n_tail = 0;
        }
        for (; n >= 16u; p += 16, n -= 16u) stripe(p);
        if (n) memcpy(tail, p, n);
        n_tail = static_cast<uint32_t>(n);
    }
    uint32_t digest() const {
        uint32_t h = total >= 16u ? rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18) : P5;
        h += static_cast<uint32_t>(total);
        const uint8_t* p = tail;
        uint32_t n = n_tail;
        for (; n >= 4u; p += 4, n -= 4u) h = rotl(h + le32(p) * P3, 17) * P4;
        for (; n; ++p, --n) h = rotl(h + *p * P5, 11) * P1;
        h ^= h >> 15, h *= P2, h ^= h >> 13, h *= P3, h ^= h >> 16;
        return h;
    }
};
inline uint32_t xxh32(const uint8_t* p, uint64_t n) {
    Xxh32 x;
    x.update(p, n);
    return x.digest();
}

// ---- the frame header
struct FrameHeader {
    uint64_t content_size;
    bool linked, block_sums, has_size, has_checksum;
    uint32_t bytes, block_max;
};
// p at a frame's magic.  kRanOut: more bytes are needed
inline uint32_t frame_header(const uint8_t* p, uint64_t n, FrameHeader& h) {
    if (n < 7u) return kRanOut;
    const uint32_t flg = p[4], bd = p[5];
    if ((flg >> 6) != 1u) return kBadVersion;
    if ((flg & 2u) || (bd & 0x8fu)) return kReservedBit;
    if (flg & 1u) return kDictionary;
    if ((bd >> 4) < 4u) return kBadBlockMax;
    h.linked = !(flg & 0x20u), h.block_sums = (flg & 0x10u) != 0, h.has_size = (flg & 8u) != 0, h.has_checksum = (flg & 4u) != 0;
    h.block_max = 1u << (8u + 2u * (bd >> 4));
    h.bytes = 7u + (h.has_size ? 8u : 0u);
    if (n < h.bytes) return kRanOut;
    h.content_size = 0;
    for (uint32_t i = 0; h.has_size && i < 8u; ++i) h.content_size |= static_cast<uint64_t>(p[6u + i]) << (8u * i);
    if (((xxh32(p + 4, h.bytes - 5u) >> 8) & 0xffu) != p[h.bytes - 1u]) return kBadHeaderChecksum;
    return kOk;
}

// ---- a compressed block's sequences
// Where a sequence's literals start in the block's text (`out`) and in the block's bytes (`lit`: they are read from
// there, never copied), and `off`: kLiteralsOnly, or the literals' length << 16 | the match's offset.  The match's length
// is what is left up to the next entry's `out`; a closing entry {text length, 0, 0} ends the list.  A literal run of more
// than kLitMost in front of a match is two entries: its first bytes as literals only, the rest with the match
struct Seq {
    uint32_t out, lit, off;
};
constexpr uint32_t kLiteralsOnly = 0xffffffffu, kLitMost = 0xfffeu;
// entries of a block of `size` bytes at most, the closing one included: a match costs 3 bytes at least, a split literal
// run 65 535; the last sequence and the closing entry
SLIMM_LZ4_HD inline uint32_t seq_bound(uint32_t size) { return size / 3u + 2u; }

// The grammar as a machine that is fed the block's bytes one at a time -- whoever holds them (the device's wave through its
// LDS ring, the host from memory) --: `pos` is the next byte it wants, which jumps over the literals.  step() returns how
// many entries it put into e[0, 3)
struct SeqWalk {
    enum State : uint32_t { Token, LitLen, Off0, Off1, MatLen, Done, Failed };
    uint32_t state = Token, status = kOk;
    uint32_t pos = 0, out = 0, matches = 0;
    uint32_t ll = 0, ml = 0, off = 0, lit_at = 0;

    // the literal length is known: the literals are passed over
    SLIMM_LZ4_HD uint32_t literals(uint32_t size, Seq* e) {
        lit_at = pos;
        if (ll > size - pos) return fail(kEndsInLiterals);
        if (ll == size - pos) {   // the last sequence
            uint32_t n = 0;
            if (ll) e[n++] = Seq{out, lit_at, kLiteralsOnly};
            out += ll, pos = size;
            e[n++] = Seq{out, 0u, 0u};
            state = Done;
            return n;
        }
        pos += ll;
        state = Off0;
        return 0;
    }
    SLIMM_LZ4_HD uint32_t match(Seq* e) {
        uint32_t n = 0;
        if (ll > kLitMost) {
            e[n++] = Seq{out, lit_at, kLiteralsOnly};
            out += ll - kLitMost, lit_at += ll - kLitMost, ll = kLitMost;
        }
        e[n++] = Seq{out, lit_at, (ll << 16) | off};
        out += ll + ml;
        ++matches;
        state = Token;
        return n;
    }
    SLIMM_LZ4_HD uint32_t fail(uint32_t cause) {
        state = Failed, status = cause;
        return 0;
    }
    // the byte at `pos` (pos < size; state below Done)
    SLIMM_LZ4_HD uint32_t step(uint8_t b, uint32_t size, Seq* e) {
        ++pos;
        switch (state) {
            case Token:
                ll = b >> 4, ml = (b & 15u) + 4u;
                if (ll == 15u) return state = LitLen, 0u;
                return literals(size, e);
            case LitLen:
                ll += b;   // (at most 255 a byte of the block: no overflow)
                return b == 255u ? 0u : literals(size, e);
            case Off0: off = b; return state = Off1, 0u;
            case Off1:
                off |= static_cast<uint32_t>(b) << 8;
                if (!off) return fail(kZeroOffset);
                if (ml == 19u) return state = MatLen, 0u;
                return match(e);
            case MatLen:
                ml += b;
                return b == 255u ? 0u : match(e);
            default: return 0u;
        }
    }
    // the block's bytes are over and the machine is not done: in words
    SLIMM_LZ4_HD uint32_t ran_off() const {
        return state == Token ? kEndsBehindMatch : state == Off0 || state == Off1 ? kEndsInOffset : kEndsInLength;
    }
};

// a block of a round (lz4_decode.hip); the host reader uses the same fields for the one block at hand
struct Block {
    uint64_t at;          // its bytes, behind the 4-byte header
    uint32_t size;
    uint32_t stored;      // 1: the bytes are the text
    uint32_t max;         // the frame's block maximum
    uint32_t frame;       // the frame of the round it belongs to
    uint64_t seq_out;     // where its seq_bound(size) entries go in the scratch
    // results (k_lz4_tokens): the text's length, the entries without the closing one, the matches among them
    uint32_t text_len, n_seq, n_match, status;
    uint64_t text_at;     // the block's text in the round's
    int64_t reach_lo;     // the lowest text position (history included) a match of it may copy from
};

}  // namespace lz4
}  // namespace slimm
