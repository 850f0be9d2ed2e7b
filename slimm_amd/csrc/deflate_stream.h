// A deflate stream inside gzip members, decoded: the part of the format the device decoder (gzip_decode.hip) and host code
// share, the same source for both.  Written from RFC 1951 / RFC 1952:
//   member  1f 8b 08 FLG MTIME(4) XFL OS, then by FLG: FEXTRA (XLEN(2) + bytes), FNAME and FCOMMENT (to a NUL), FHCRC (2);
//           the deflate blocks; CRC32 of the text, ISIZE = its length mod 2^32; members may follow each other
//   block   BFINAL(1) BTYPE(2), bits LSB first: 0 stored (to a byte, LEN, NLEN = ~LEN, LEN bytes), 1 fixed codes,
//           2 dynamic codes (HLIT(5) HDIST(5) HCLEN(4), the code-length code's lengths in a fixed order, the HLIT + 257
//           + HDIST + 1 lengths of the two codes, run-length coded), then symbols: a literal, the end of the block, or
//           a length (3..258) with a distance (1..32768) back into the text
// A block may start at any bit, and a copy may reach the 32 768 bytes in front of it whatever block they came from: a
// decoder that starts at a block in the middle of a member (a CHUNK) writes what it cannot fill as a MARKER that names the
// byte of those 32 768 it wants (Out16 below), and the markers are resolved once the chunk in front has its text.
// The checks are zlib's (inflate.c), so that what zlib refuses is refused here: code sets over-subscribed, or incomplete
// unless they have a single code of one bit; no code for the end of the block; a repeat with no length in front.
#pragma once
#include <stdint.h>

#if defined(__host__) && defined(__device__)
#define SLIMM_GZ_HD __host__ __device__
#else
#define SLIMM_GZ_HD
#endif

namespace slimm {
namespace gz {

constexpr uint32_t kWindow = 32768;      // how far back a copy may reach
constexpr uint16_t kMarker = 0x8000u;    // Out16: kMarker | i = byte i of the 32 768 in front of the chunk

enum Status : uint32_t {
    kOk = 0,
    kRanOut,          // the bytes at hand end inside the block (more may come)
    kBadBlockType,
    kBadStoredLength,
    kTooManySymbols,
    kBadCodeLengths,
    kBadRepeat,
    kNoEndOfBlock,
    kBadLitLengths,
    kBadDistLengths,
    kBadCode,
    kBadDistCode,
    kTooFarBack,
    kOverrun,         // more text than the size pass counted (never: a guard of the buffers)
    kBadCrc,
    kBadLength,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "invalid block type",
                                                "invalid stored block lengths",
                                                "too many length or distance symbols",
                                                "invalid code lengths set",
                                                "invalid bit length repeat",
                                                "invalid code -- missing end-of-block",
                                                "invalid literal/lengths set",
                                                "invalid distances set",
                                                "invalid literal/length code",
                                                "invalid distance code",
                                                "invalid distance too far back",
                                                "text longer than counted",
                                                "incorrect data check",
                                                "incorrect length check"};
    return s < kStatusCount ? t[s] : "unknown error";
}

// LSB-first bit reader over bytes[0, end_byte): at most 32 bits a call
struct Bits {
    const uint8_t* p;
    uint64_t next, end;   // next byte to load, bytes at hand
    uint64_t acc;         // n bits not handed out yet, the next one lowest
    uint32_t n;
    SLIMM_GZ_HD Bits(const uint8_t* bytes, uint64_t bit, uint64_t end_byte) : p(bytes), next(bit >> 3), end(end_byte), acc(0), n(0) {
        uint32_t drop = static_cast<uint32_t>(bit & 7u), v;
        if (drop) (void)get(drop, v);
    }
    SLIMM_GZ_HD uint64_t pos() const { return next * 8u - n; }
    SLIMM_GZ_HD bool fill(uint32_t k) {
        while (n < k) {
            if (next >= end) return false;
            acc |= static_cast<uint64_t>(p[next++]) << n;
            n += 8;
        }
        return true;
    }
    SLIMM_GZ_HD bool get(uint32_t k, uint32_t& v) {
        if (!fill(k)) return false;
        v = static_cast<uint32_t>(acc & ((1ull << k) - 1u));
        acc >>= k;
        n -= k;
        return true;
    }
    SLIMM_GZ_HD void to_byte() {   // the bits up to the next byte boundary dropped
        const uint32_t k = n & 7u;
        acc >>= k;
        n -= k;
    }
};

// A canonical Huffman code: how many codes of each length, and the symbols in the code's order
struct Huff {
    uint16_t count[16];
    uint16_t symbol[288];
};
struct DistHuff {
    uint16_t count[16];
    uint16_t symbol[32];
};
// one decoder's tables (1 KiB: LDS on the device)
struct Tables {
    Huff lit;
    DistHuff dist;
    uint8_t len[320];
};

// count / symbol from n code lengths.  Returns what is left of the code space: 0 a complete code, > 0 an incomplete
// one, < 0 an over-subscribed one; *max_len: the longest code
template <typename H>
SLIMM_GZ_HD int build(H& h, const uint8_t* len, uint32_t n, uint32_t* max_len) {
    uint16_t offs[16];
    for (uint32_t l = 0; l < 16; ++l) h.count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++h.count[len[s]];
    uint32_t mx = 15;
    while (mx > 0 && h.count[mx] == 0) --mx;
    *max_len = mx;
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = static_cast<uint16_t>(offs[l] + h.count[l]);
    for (uint32_t s = 0; s < n; ++s)
        if (len[s]) h.symbol[offs[len[s]]++] = static_cast<uint16_t>(s);
    return left;
}

// the next symbol of code h: kOk, kRanOut, or kBadCode (bits that are no code of an incomplete set)
template <typename H>
SLIMM_GZ_HD uint32_t decode(Bits& b, const H& h, uint32_t& sym) {
    (void)b.fill(15);   // (near the end of the bytes fewer: the loop asks bit by bit)
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        if (b.n == 0 && !b.fill(1)) return kRanOut;
        code |= static_cast<int>(b.acc & 1u);
        b.acc >>= 1;
        --b.n;
        const int cnt = h.count[l];
        if (code - cnt < first) {
            sym = h.symbol[index + (code - first)];
            return kOk;
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return kBadCode;
}

// The two codes of a dynamic block, from behind its 3 header bits on.  strict: what a block CANDIDATE must pass on top of
// zlib's checks (a literal/length code that is complete)
SLIMM_GZ_HD inline uint32_t read_dynamic(Bits& b, Tables& t, bool strict) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hlit, hdist, hclen, v, mx;
    if (!b.get(5, hlit) || !b.get(5, hdist) || !b.get(4, hclen)) return kRanOut;
    if (hlit > 29u || hdist > 29u) return kTooManySymbols;
    hlit += 257u, hdist += 1u, hclen += 4u;
    for (uint32_t i = 0; i < 19; ++i) t.len[order[i]] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        if (!b.get(3, v)) return kRanOut;
        t.len[order[i]] = static_cast<uint8_t>(v);
    }
    // (the code-length code in the distance code's room: 19 symbols)
    if (build(t.dist, t.len, 19, &mx) != 0) return kBadCodeLengths;
    uint32_t i = 0;
    const uint32_t total = hlit + hdist;
    while (i < total) {
        uint32_t sym;
        const uint32_t st = decode(b, t.dist, sym);
        if (st != kOk) return st == kBadCode ? kBadCodeLengths : st;
        if (sym < 16u) {
            t.len[i++] = static_cast<uint8_t>(sym);
            continue;
        }
        uint32_t prev = 0, rep;
        if (sym == 16u) {
            if (i == 0) return kBadRepeat;
            prev = t.len[i - 1];
            if (!b.get(2, rep)) return kRanOut;
            rep += 3u;
        } else if (sym == 17u) {
            if (!b.get(3, rep)) return kRanOut;
            rep += 3u;
        } else {
            if (!b.get(7, rep)) return kRanOut;
            rep += 11u;
        }
        if (i + rep > total) return kBadRepeat;
        while (rep--) t.len[i++] = static_cast<uint8_t>(prev);
    }
    if (t.len[256] == 0) return kNoEndOfBlock;
    int left = build(t.lit, t.len, hlit, &mx);
    if (left < 0 || (left > 0 && (strict || mx != 1u))) return kBadLitLengths;
    left = build(t.dist, t.len + hlit, hdist, &mx);
    if (left < 0 || (left > 0 && mx > 1u)) return kBadDistLengths;
    return kOk;
}

SLIMM_GZ_HD inline void fixed_codes(Tables& t) {
    uint32_t mx;
    for (uint32_t s = 0; s < 288; ++s) t.len[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    (void)build(t.lit, t.len, 288, &mx);
    for (uint32_t s = 0; s < 30; ++s) t.len[s] = 5;
    (void)build(t.dist, t.len, 30, &mx);
}

// Where a decoder's text goes.  Count: nowhere, its bytes counted (the size pass)
struct Count {
    uint64_t n = 0;
    SLIMM_GZ_HD uint32_t literal(uint32_t) {
        ++n;
        return kOk;
    }
    SLIMM_GZ_HD uint32_t copy(uint32_t len, uint32_t) {
        n += len;
        return kOk;
    }
};
// Out16: 16 bits per byte of text -- the byte, or a marker for a byte of the `avail` (<= 32 768) bytes of the member in
// front of the chunk; a copy of a marker is that marker.  At most cap bytes of text
struct Out16 {
    uint16_t* out;
    uint64_t n, cap;
    uint32_t avail;
    SLIMM_GZ_HD uint32_t literal(uint32_t v) {
        if (n >= cap) return kOverrun;
        out[n++] = static_cast<uint16_t>(v);
        return kOk;
    }
    SLIMM_GZ_HD uint32_t copy(uint32_t len, uint32_t dist) {
        if (n + len > cap) return kOverrun;
        if (dist > n && dist - n > avail) return kTooFarBack;
        uint32_t k = 0;
        for (; k < len && dist > n; ++k, ++n)   // (the source lies in front of the chunk)
            out[n] = static_cast<uint16_t>(kMarker | (kWindow - static_cast<uint32_t>(dist - n)));
        // the rest eight at a time, read before any of them is written: a load's latency per eight, not per one (a source
        // that overlaps its copy, dist < 8, repeats its dist symbols, read once)
        uint16_t v[8];
        if (k < len && dist < 8u) {
            for (uint32_t j = 0; j < 8u; ++j) v[j] = j < dist ? out[n - dist + j] : uint16_t(0);
            for (uint32_t j = 0; k < len; ++k, ++n) {
                out[n] = v[j];
                j = j + 1u == dist ? 0u : j + 1u;
            }
        }
        while (k < len) {
            const uint32_t m = len - k < 8u ? len - k : 8u;
            const uint16_t* src = out + (n - dist);
            for (uint32_t j = 0; j < 8u; ++j) v[j] = j < m ? src[j] : uint16_t(0);
            for (uint32_t j = 0; j < 8u; ++j)
                if (j < m) out[n + j] = v[j];
            n += m;
            k += m;
        }
        return kOk;
    }
};

// One block from its first bit on: *final = its BFINAL.  kinds[3], when given, counts the block by its type
template <typename Sink>
SLIMM_GZ_HD uint32_t inflate_block(Bits& b, Tables& t, Sink& out, bool* final, uint32_t* kinds) {
    uint32_t fin, type, v;
    if (!b.get(1, fin) || !b.get(2, type)) return kRanOut;
    *final = fin != 0;
    if (type == 3u) return kBadBlockType;
    if (type == 0u) {
        uint32_t len, nlen;
        b.to_byte();
        if (!b.get(16, len) || !b.get(16, nlen)) return kRanOut;
        if ((len ^ 0xffffu) != nlen) return kBadStoredLength;
        if (b.pos() / 8u + len > b.end) return kRanOut;
        for (uint32_t k = 0; k < len; ++k) {
            (void)b.get(8, v);
            const uint32_t st = out.literal(v);
            if (st != kOk) return st;
        }
        if (kinds) ++kinds[0];
        return kOk;
    }
    if (type == 1u) {
        fixed_codes(t);
    } else {
        const uint32_t st = read_dynamic(b, t, false);
        if (st != kOk) return st;
    }
    for (;;) {
        uint32_t sym;
        uint32_t st = decode(b, t.lit, sym);
        if (st != kOk) return st;
        if (sym < 256u) {
            st = out.literal(sym);
            if (st != kOk) return st;
            continue;
        }
        if (sym == 256u) break;
        sym -= 257u;
        if (sym >= 29u) return kBadCode;
        uint32_t len, extra = 0;
        if (sym < 8u) {
            len = 3u + sym;
        } else if (sym == 28u) {
            len = 258u;
        } else {
            const uint32_t e = (sym - 4u) >> 2;
            if (!b.get(e, extra)) return kRanOut;
            len = 3u + ((4u + (sym & 3u)) << e) + extra;
        }
        uint32_t ds, dist;
        st = decode(b, t.dist, ds);
        if (st != kOk) return st == kBadCode ? kBadDistCode : st;
        if (ds >= 30u) return kBadDistCode;
        if (ds < 4u) {
            dist = 1u + ds;
        } else {
            const uint32_t e = (ds - 2u) >> 1;
            if (!b.get(e, extra)) return kRanOut;
            dist = 1u + ((2u + (ds & 1u)) << e) + extra;
        }
        st = out.copy(len, dist);
        if (st != kOk) return st;
    }
    if (kinds) ++kinds[type];
    return kOk;
}

// A chunk start's size pass (gzip_decode.hip: k_gz_walk): where the walk ended -- on a later chunk start, behind a final
// block, on the first block boundary behind kChunkTextSoft bytes of text (status kOk), or, when the bytes ran out
// (kRanOut), the last whole block boundary it passed -- and the text up to there
struct Walk {
    uint64_t end_bit, n;
    uint32_t status, final;
};
// A chunk of the chain for the decode pass: blocks [start_bit, stop_bit) of the bytes at hand give len bytes of text, at
// text_at of the round's text, with avail (<= 32 768) bytes of its member in front; its pieces (kPiece bytes of text
// each, for the CRC) start at piece0, the last one's x^(8 bytes); and what decoding and resolving found
struct Chunk {
    uint64_t start_bit, stop_bit, text_at, len;
    uint32_t avail, piece0, last_mul, status;
    uint32_t crc, kinds[3];
    uint64_t markers;
};
constexpr uint32_t kPiece = 2048;

// Does a non-final dynamic block that zlib would take plausibly start at `bit`?  cheap: the 17 header bits and the Kraft
// sum of the code-length code alone (registers only); the rest: is_candidate
SLIMM_GZ_HD inline bool cheap_candidate(const uint8_t* bytes, uint64_t bit, uint64_t end_byte) {
    Bits b(bytes, bit, end_byte);
    uint32_t v, hlit, hdist, hclen;
    if (!b.get(3, v) || v != 4u) return false;   // BFINAL = 0, BTYPE = 2 (its low bit first)
    if (!b.get(5, hlit) || !b.get(5, hdist) || !b.get(4, hclen)) return false;
    if (hlit > 29u || hdist > 29u) return false;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < hclen + 4u; ++i) {
        if (!b.get(3, v)) return false;
        if (v) kraft += 128u >> v;
    }
    return kraft == 128u;
}
SLIMM_GZ_HD inline bool is_candidate(const uint8_t* bytes, uint64_t bit, uint64_t end_byte, Tables& t) {
    Bits b(bytes, bit, end_byte);
    uint32_t v;
    if (!b.get(3, v) || v != 4u) return false;
    return read_dynamic(b, t, true) == kOk;
}

// CRC-32 as gzip takes it (reflected, polynomial 0xedb88320), in pieces: raw(A) is the register after A's bytes from a
// register of 0, which is linear -- raw(A B) = raw(A) * x^(8 |B|) + raw(B) mod P -- so pieces are summed in any order,
// and the member's register s (0xffffffff at its start, the CRC its complement) steps over a piece as
// s * x^(8 |B|) + raw(B).  Polynomials have their x^0 coefficient in bit 31.
SLIMM_GZ_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
SLIMM_GZ_HD inline uint32_t crc_x_pow8(uint64_t n_bytes) {   // x^(8 n) mod P
    uint32_t p = 1u << 31, sq = 1u << 23;   // sq = x^8
    for (; n_bytes; n_bytes >>= 1) {
        if (n_bytes & 1u) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
    }
    return p;
}
SLIMM_GZ_HD inline uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
    return c;
}

// A member header at p[0, n): its length; 0: more bytes are needed; -1: no gzip member starts here
inline long member_header(const uint8_t* p, uint64_t n) {
    if (n >= 1 && p[0] != 0x1f) return -1;
    if (n >= 2 && p[1] != 0x8b) return -1;
    if (n >= 3 && p[2] != 8) return -1;
    if (n >= 4 && (p[3] & 0xe0u)) return -1;
    if (n < 10) return 0;
    const uint32_t flg = p[3];
    uint64_t at = 10;
    if (flg & 4u) {
        if (n < at + 2) return 0;
        at += 2u + (p[at] | (static_cast<uint32_t>(p[at + 1]) << 8));
        if (n < at) return 0;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1) {   // FNAME, FCOMMENT
        if (!(flg & f)) continue;
        while (at < n && p[at]) ++at;
        if (at >= n) return 0;
        ++at;
    }
    if (flg & 2u) at += 2;
    if (n < at) return 0;
    return static_cast<long>(at);
}

}  // namespace gz
}  // namespace slimm
