// The zstd frame format: the part both the host reader (host/zstd.cpp) and the device decoder (zstd_decode.hip) run, the
// same source for both.  Written from the format as zstd writes it (RFC 8878):
//   frame     magic 28 B5 2F FD, a descriptor byte (content size flag 2 bits, single segment, -, reserved, checksum,
//             dictionary id flag 2 bits), a window descriptor unless single segment (exponent 5 bits, mantissa 3:
//             window = (1 + mantissa / 8) << (10 + exponent)), a dictionary id of 0 / 1 / 2 / 4 bytes, a content size of
//             0 / 1 / 2 (+ 256) / 4 / 8 bytes, blocks, and the low 32 bits of the text's XXH64 when the descriptor says so
//   skippable magic 0x184D2A5?, a 4-byte length, that many bytes
//   block     3 bytes: last (1 bit), type (2: raw, RLE, compressed, reserved), size (21); at most min(window, 128 KiB) of
//             text -- and of content -- each
//   compressed block = a literals section (raw, RLE, or Huffman-coded in 1 or 4 streams read BACKWARDS from a padding bit,
//             with the code's weights in front, direct or FSE-coded, or "treeless": the frame's last code again) and a
//             sequences section: a count, three FSE tables (literal lengths, offsets, match lengths; each predefined, one
//             symbol, described, or the frame's last again) and one backward bitstream of three interleaved states.  A
//             sequence = copy `literal length` literals, then `match length` bytes from `offset` back, where offset values
//             1..3 name the three most recent offsets (shifted by one when the literal length is 0; "3" is then the most
//             recent one minus 1), which a frame starts at 1, 4, 8
// Everything that loops here is counted by a size the headers state; nothing indexes outside what it is given.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__host__) && defined(__device__)
#define SLIMM_ZS_HD __host__ __device__
#else
#define SLIMM_ZS_HD
#endif

namespace slimm {
namespace zs {

constexpr uint32_t kMagic = 0xFD2FB528u, kSkippable = 0x184D2A50u;
constexpr uint32_t kBlockMax = 128u << 10;
constexpr uint64_t kWindowMax = 1ull << 27;   // 128 MiB: what `zstd -d` takes without --long
constexpr uint32_t kHufLogMax = 11, kLLLogMax = 9, kOFLogMax = 8, kMLLogMax = 9, kWeightLogMax = 6;
constexpr uint32_t kMaxLL = 35, kMaxML = 52, kMaxOF = 31, kMaxWeight = 12;
constexpr uint32_t kOffsetCodeMax = 28;       // (an offset of at most kWindowMax + 3 has a code of at most 27)
constexpr uint32_t kHufDescMax = 129;         // a Huffman description: its header byte and at most 128 bytes
constexpr uint32_t kPad = 8;                  // zeroed bytes behind a buffer that the readers may load (never use)

enum Status : uint32_t {
    kOk = 0,
    kRanOut,
    kNoFrame,
    kReservedBit,
    kDictionary,
    kWindowTooLarge,
    kReservedBlock,
    kBlockTooLarge,
    kBadLiteralsHeader,
    kBadWeights,
    kBadFse,
    kBadPadding,
    kBadLiterals,
    kBadSequences,
    kNoTable,
    kBadOffset,
    kBadContentSize,
    kBadChecksum,
    kBadCode,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "bytes behind the last frame that start no frame",
                                                "a reserved bit is set",
                                                "a dictionary is needed: not supported",
                                                "a window of more than 128 MiB: refused (zstd --long)",
                                                "reserved block type",
                                                "a block larger than its maximum",
                                                "a literals section larger than its block",
                                                "bad Huffman weights",
                                                "bad FSE table description",
                                                "a bitstream that does not end on its padding bit",
                                                "literals total disagrees with the block",
                                                "sequence total disagrees with the block",
                                                "a repeated table with none in front to repeat",
                                                "an offset beyond the frame's start or window",
                                                "content size mismatch",
                                                "content checksum mismatch",
                                                "bad sequence code"};
    return s < kStatusCount ? t[s] : "unknown error";
}

SLIMM_ZS_HD inline uint32_t high_bit(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); }   // v != 0

// 8 bytes from p[at] on, little-endian; bytes at or behind `len` read as 0
SLIMM_ZS_HD inline uint64_t load64(const uint8_t* p, uint64_t at, uint64_t len) {
    uint64_t v = 0;
    if (at + 8u <= len) {
        for (uint32_t i = 0; i < 8u; ++i) v |= static_cast<uint64_t>(p[at + i]) << (8u * i);
    } else {
        for (uint32_t i = 0; at + i < len; ++i) v |= static_cast<uint64_t>(p[at + i]) << (8u * i);
    }
    return v;
}
SLIMM_ZS_HD inline uint32_t le16(const uint8_t* p) { return p[0] | (static_cast<uint32_t>(p[1]) << 8); }
SLIMM_ZS_HD inline uint32_t le24(const uint8_t* p) { return le16(p) | (static_cast<uint32_t>(p[2]) << 16); }
SLIMM_ZS_HD inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// A bitstream read from its END: the last byte's highest set bit is the padding mark; bits in front of the stream's first
// read as 0 (`off` goes negative: the streams' end checks are on it).  At most 32 bits a call
struct BackBits {
    const uint8_t* p;
    uint64_t len;
    int64_t off;   // bits [0, off) are still to read
    SLIMM_ZS_HD bool init(const uint8_t* bytes, uint64_t n) {
        p = bytes, len = n, off = 0;
        if (!n || !bytes[n - 1]) return false;
        off = static_cast<int64_t>(n * 8u) - (8 - static_cast<int64_t>(high_bit(bytes[n - 1])));
        return true;
    }
    SLIMM_ZS_HD uint32_t read(uint32_t k) {
        off -= k;
        if (!k) return 0;
        const uint64_t mask = (1ull << k) - 1u;
        if (off >= 0) return static_cast<uint32_t>((load64(p, static_cast<uint64_t>(off) >> 3, len) >> (off & 7)) & mask);
        const int64_t shift = -off;
        if (shift >= static_cast<int64_t>(k)) return 0;
        return static_cast<uint32_t>((load64(p, 0, len) << shift) & mask);
    }
};

// ---- FSE
// A table description (forward, LSB first) -> norm[0, n_sym): the symbols' shares of 1 << log (-1: "less than one")
SLIMM_ZS_HD inline uint32_t fse_read_desc(const uint8_t* p, uint64_t len, uint32_t max_log, uint32_t max_sym, int16_t* norm, uint32_t& log,
                                           uint32_t& n_sym, uint32_t& bytes) {
    uint64_t pos = 0;
    auto get = [&](uint32_t k) {
        const uint32_t v = static_cast<uint32_t>((load64(p, pos >> 3, len) >> (pos & 7u)) & ((1ull << k) - 1u));
        pos += k;
        return v;
    };
    log = get(4) + 5u;
    if (log > max_log) return kBadFse;
    int32_t remaining = 1 << log;
    uint32_t symb = 0;
    while (remaining > 0 && symb <= max_sym) {
        const uint32_t bits = high_bit(static_cast<uint32_t>(remaining) + 1u) + 1u;
        uint32_t val = get(bits);
        const uint32_t lower = (1u << (bits - 1u)) - 1u, threshold = (1u << bits) - 1u - (static_cast<uint32_t>(remaining) + 1u);
        if ((val & lower) < threshold) {
            --pos;
            val &= lower;
        } else if (val > lower) {
            val -= threshold;
        }
        const int32_t proba = static_cast<int32_t>(val) - 1;
        remaining -= proba < 0 ? 1 : proba;
        norm[symb++] = static_cast<int16_t>(proba);
        if (proba == 0) {
            for (;;) {   // (each turn takes 2 bits of at most len * 8 + 64: counted by `pos`)
                const uint32_t rep = get(2);
                for (uint32_t i = 0; i < rep && symb <= max_sym; ++i) norm[symb++] = 0;
                if (rep != 3u || symb > max_sym || pos > len * 8u) break;
            }
        }
        if (pos > len * 8u) return kBadFse;
    }
    if (remaining != 0 || symb > max_sym + 1u || pos > len * 8u) return kBadFse;
    n_sym = symb;
    bytes = static_cast<uint32_t>((pos + 7u) >> 3);
    return kOk;
}

// norm -> the decoding table, 1 << log entries of {symbol 8, bits to read 8, next state's base 16}
SLIMM_ZS_HD inline uint32_t fse_entry_sym(uint32_t e) { return e & 255u; }
SLIMM_ZS_HD inline uint32_t fse_entry_bits(uint32_t e) { return (e >> 8) & 255u; }
SLIMM_ZS_HD inline uint32_t fse_entry_base(uint32_t e) { return e >> 16; }
SLIMM_ZS_HD inline uint32_t fse_build(const int16_t* norm, uint32_t n_sym, uint32_t log, uint32_t* table) {
    const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    uint16_t next[64];
    if (n_sym > 64u) return kBadFse;
    uint32_t high = size;
    for (uint32_t s = 0; s < n_sym; ++s)
        if (norm[s] == -1) {
            if (!high) return kBadFse;
            table[--high] = s;
            next[s] = 1;
        }
    uint32_t pos = 0, placed = size - high;
    for (uint32_t s = 0; s < n_sym; ++s) {
        if (norm[s] <= 0) continue;
        next[s] = static_cast<uint16_t>(norm[s]);
        placed += static_cast<uint32_t>(norm[s]);
        if (placed > size) return kBadFse;
        for (int32_t i = 0; i < norm[s]; ++i) {
            table[pos] = s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    if (pos != 0 || placed != size) return kBadFse;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t s = table[i], x = next[s]++;
        const uint32_t nb = log - high_bit(x);
        table[i] = s | (nb << 8) | (((x << nb) - size) << 16);
    }
    return kOk;
}

// the three predefined distributions (literal lengths and match lengths: 64 states, offsets: 32)
SLIMM_ZS_HD inline uint32_t predefined(uint32_t which, int16_t* norm, uint32_t& log) {
    const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    const int8_t* src = which == 0 ? ll : which == 1 ? of : ml;
    const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
    for (uint32_t i = 0; i < n; ++i) norm[i] = src[i];
    log = which == 1 ? 5u : 6u;
    return n;
}
// code -> baseline and extra bits, for literal lengths and match lengths
SLIMM_ZS_HD inline void ll_code(uint32_t c, uint32_t& base, uint32_t& bits) {
    const uint32_t b[20] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    const uint8_t n[20] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    if (c < 16u) base = c, bits = 0;
    else
        base = b[c - 16u], bits = n[c - 16u];
}
SLIMM_ZS_HD inline void ml_code(uint32_t c, uint32_t& base, uint32_t& bits) {
    const uint32_t b[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    const uint8_t n[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    if (c < 32u) base = c + 3u, bits = 0;
    else
        base = b[c - 32u], bits = n[c - 32u];
}

// A sequence table of a block: predefined, one symbol (at `at`), or described (at `at`, at most `len` bytes of it)
enum TableKind : uint32_t { kPredefined = 0, kRle = 1, kFse = 2, kRepeat = 3 };
struct TableRef {
    uint32_t kind, len;
    uint64_t at;
};
// which: 0 literal lengths, 1 offsets, 2 match lengths.  table: 1 << max log entries
SLIMM_ZS_HD inline uint32_t seq_table(const uint8_t* base, const TableRef& r, uint32_t which, uint32_t* table, uint32_t& log, uint32_t* used = nullptr) {
    const uint32_t max_log = which == 1 ? kOFLogMax : which == 0 ? kLLLogMax : kMLLogMax;
    const uint32_t max_sym = which == 1 ? kMaxOF : which == 0 ? kMaxLL : kMaxML;
    int16_t norm[64];
    uint32_t n_sym = 0, bytes = 0;
    if (r.kind == kRle) {
        if (r.len < 1u) return kRanOut;
        if (base[r.at] > max_sym) return kBadCode;
        table[0] = base[r.at];
        log = 0;
        if (used) *used = 1;
        return kOk;
    }
    if (r.kind == kPredefined) n_sym = predefined(which, norm, log);
    else if (r.kind == kFse) {
        const uint32_t st = fse_read_desc(base + r.at, r.len, max_log, max_sym, norm, log, n_sym, bytes);
        if (st != kOk) return st;
    } else {
        return kNoTable;
    }
    if (used) *used = bytes;
    return fse_build(norm, n_sym, log, table);
}

// ---- Huffman
// The description at p -> weights w[0, n_w) (the last symbol's weight is implied: huf_build); fse_tmp: 64 entries
SLIMM_ZS_HD inline uint32_t huf_read_weights(const uint8_t* p, uint64_t len, uint8_t* w, uint32_t& n_w, uint32_t& bytes, uint32_t* fse_tmp) {
    if (len < 1u) return kBadWeights;
    const uint32_t hb = p[0];
    if (hb >= 128u) {
        n_w = hb - 127u;
        bytes = 1u + (n_w + 1u) / 2u;
        if (bytes > len) return kBadWeights;
        for (uint32_t i = 0; i < n_w; ++i) w[i] = (i & 1u) ? (p[1u + i / 2u] & 15u) : (p[1u + i / 2u] >> 4);
        return kOk;
    }
    bytes = 1u + hb;
    if (bytes > len || hb < 2u) return kBadWeights;
    int16_t norm[16];
    uint32_t log = 0, n_sym = 0, used = 0;
    if (fse_read_desc(p + 1, hb, kWeightLogMax, kMaxWeight, norm, log, n_sym, used) != kOk) return kBadWeights;
    if (used >= hb || fse_build(norm, n_sym, log, fse_tmp) != kOk) return kBadWeights;
    BackBits b;
    if (!b.init(p + 1u + used, hb - used)) return kBadWeights;
    uint32_t s1 = b.read(log), s2 = b.read(log), n = 0;
    bool ended = false;
    while (n < 254u) {   // (two weights a turn, 255 at most)
        w[n++] = static_cast<uint8_t>(fse_entry_sym(fse_tmp[s1]));
        s1 = fse_entry_base(fse_tmp[s1]) + b.read(fse_entry_bits(fse_tmp[s1]));
        if (b.off < 0) {
            w[n++] = static_cast<uint8_t>(fse_entry_sym(fse_tmp[s2]));
            ended = true;
            break;
        }
        w[n++] = static_cast<uint8_t>(fse_entry_sym(fse_tmp[s2]));
        s2 = fse_entry_base(fse_tmp[s2]) + b.read(fse_entry_bits(fse_tmp[s2]));
        if (b.off < 0) {
            w[n++] = static_cast<uint8_t>(fse_entry_sym(fse_tmp[s1]));
            ended = true;
            break;
        }
    }
    if (!ended) return kBadWeights;
    n_w = n;
    return kOk;
}
// weights -> the decoding table, 1 << log entries of {symbol 8, code length 8}; w has room for one more weight
SLIMM_ZS_HD inline uint32_t huf_build(uint8_t* w, uint32_t n_w, uint16_t* table, uint32_t& log) {
    uint32_t sum = 0;
    if (n_w < 1u || n_w > 255u) return kBadWeights;
    for (uint32_t i = 0; i < n_w; ++i) {
        if (w[i] > kHufLogMax) return kBadWeights;
        sum += w[i] ? 1u << (w[i] - 1u) : 0u;
    }
    if (!sum) return kBadWeights;
    log = high_bit(sum) + 1u;
    if (log > kHufLogMax) return kBadWeights;
    const uint32_t left = (1u << log) - sum;
    if (left & (left - 1u)) return kBadWeights;
    w[n_w] = static_cast<uint8_t>(high_bit(left) + 1u);
    const uint32_t n = n_w + 1u;
    uint32_t count[kHufLogMax + 2u] = {}, idx[kHufLogMax + 2u] = {};
    for (uint32_t i = 0; i < n; ++i)
        if (w[i]) ++count[log + 1u - w[i]];
    idx[log] = 0;   // (the longest codes come first)
    for (uint32_t b = log; b >= 1u; --b) idx[b - 1u] = idx[b] + count[b] * (1u << (log - b));
    if (idx[0] != (1u << log)) return kBadWeights;
    for (uint32_t i = 0; i < n; ++i) {
        if (!w[i]) continue;
        const uint32_t nb = log + 1u - w[i], span = 1u << (log - nb);
        for (uint32_t k = 0; k < span; ++k) table[idx[nb] + k] = static_cast<uint16_t>(i | (nb << 8));
        idx[nb] += span;
    }
    return kOk;
}
// one stream -> exactly `count` bytes
SLIMM_ZS_HD inline uint32_t huf_decode_stream(const uint8_t* p, uint64_t len, const uint16_t* table, uint32_t log, uint8_t* out, uint32_t count) {
    BackBits b;
    if (!b.init(p, len)) return kBadPadding;
    const uint32_t mask = (1u << log) - 1u;
    uint32_t state = b.read(log);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = table[state], nb = e >> 8;
        out[i] = static_cast<uint8_t>(e);
        state = ((state << nb) | b.read(nb)) & mask;
    }
    return b.off == -static_cast<int64_t>(log) ? kOk : kBadLiterals;
}

// ---- a block's sections
struct LitHeader {
    uint32_t type;      // 0 raw, 1 RLE, 2 Huffman with its description, 3 treeless
    uint32_t regen, comp, streams, bytes;   // (comp: the section's bytes behind its header)
};
inline uint32_t literals_header(const uint8_t* p, uint64_t len, LitHeader& h) {
    if (len < 1u) return kBadLiteralsHeader;
    h.type = p[0] & 3u;
    const uint32_t fmt = (p[0] >> 2) & 3u;
    h.streams = 1;
    if (h.type < 2u) {
        h.bytes = fmt == 1u ? 2u : fmt == 3u ? 3u : 1u;
        if (len < h.bytes) return kBadLiteralsHeader;
        h.regen = h.bytes == 1u ? p[0] >> 3 : h.bytes == 2u ? le16(p) >> 4 : le24(p) >> 4;
        h.comp = h.type == 0u ? h.regen : 1u;
    } else {
        h.bytes = fmt < 2u ? 3u : fmt + 2u;
        if (len < h.bytes) return kBadLiteralsHeader;
        const uint64_t v = load64(p, 0, h.bytes) >> 4;
        const uint32_t n = fmt < 2u ? 10u : fmt == 2u ? 14u : 18u;
        h.regen = static_cast<uint32_t>(v & ((1u << n) - 1u));
        h.comp = static_cast<uint32_t>((v >> n) & ((1u << n) - 1u));
        h.streams = fmt == 0u ? 1u : 4u;
    }
    if (h.regen > kBlockMax || static_cast<uint64_t>(h.bytes) + h.comp > len) return kBadLiteralsHeader;
    return kOk;
}
struct SeqHeader {
    uint32_t n_seq, mode[3], bytes;   // mode: of literal lengths, offsets, match lengths
};
inline uint32_t sequences_header(const uint8_t* p, uint64_t len, SeqHeader& h) {
    if (len < 1u) return kBadSequences;
    h.mode[0] = h.mode[1] = h.mode[2] = 0;
    if (p[0] == 0u) {
        h.n_seq = 0, h.bytes = 1;
        return len == 1u ? kOk : kBadSequences;   // (nothing lies behind a count of 0)
    }
    if (p[0] < 128u) h.n_seq = p[0], h.bytes = 1;
    else if (p[0] < 255u) {
        if (len < 2u) return kBadSequences;
        h.n_seq = ((p[0] - 128u) << 8) + p[1], h.bytes = 2;
    } else {
        if (len < 3u) return kBadSequences;
        h.n_seq = le16(p + 1) + 0x7f00u, h.bytes = 3;
    }
    if (len < h.bytes + 1u) return kBadSequences;
    const uint32_t m = p[h.bytes++];
    if (m & 3u) return kReservedBit;
    h.mode[0] = m >> 6, h.mode[1] = (m >> 4) & 3u, h.mode[2] = (m >> 2) & 3u;
    return kOk;
}

// A block as the plan leaves it: where its parts lie in the buffer (`base` + ...), what decoding needs, where its results go
enum BlockType : uint32_t { kRaw = 0, kRleBlock = 1, kCompressed = 2 };
struct Block {
    uint64_t at;             // the block's content
    uint32_t size, type;     // content bytes (RLE: 1); BlockType
    uint32_t max;            // the frame's Block_Maximum_Size
    uint32_t regen;          // raw / RLE: the text's bytes; compressed: after decoding
    // compressed: the literals
    uint32_t lit_type, lit_regen, lit_streams;
    uint64_t lit_at;         // raw: the bytes, RLE: the byte, Huffman: the streams (4: the jump table first)
    uint32_t lit_len;        // ... and their bytes
    uint64_t huf_at;         // the Huffman description (treeless: the copy of the one repeated)
    uint32_t huf_len;
    uint32_t n_seq;
    TableRef table[3];
    uint64_t bits_at;        // the sequences' bitstream
    uint32_t bits_len;
    uint64_t lit_out, seq_out;   // where the decoded literals and the n_seq + 1 sequences go in the scratch
    // results
    uint32_t status;
    uint32_t rep[3];         // the repeat offsets behind the block, in terms of those in front (sym_*), or plain
    uint64_t text_at;        // the block's text in the round's
    int64_t reach_lo;        // the lowest text position (history included) a match of it may copy from
    uint32_t entry[3];       // the repeat offsets in front of it, plain (behind the composition)
    uint32_t window;         // the frame's window
    uint32_t frame, pad;     // the frame of the round it belongs to
};
// a sequence: where its literals start in the block's text and in the block's literals, its offset (plain or symbolic);
// entry n_seq closes the last one
struct Seq {
    uint32_t out, lit, off;
};

// repeat offsets "slot i of those in front of the block, minus k"
constexpr uint32_t kSym = 0x80000000u;
SLIMM_ZS_HD inline uint32_t sym(uint32_t slot) { return kSym | (slot << 28); }
SLIMM_ZS_HD inline bool is_sym(uint32_t v) { return (v & kSym) != 0; }
// v with the offsets in front put in; 0: no offset (corrupt)
SLIMM_ZS_HD inline uint32_t substitute(uint32_t v, const uint32_t entry[3]) {
    if (!is_sym(v)) return v;
    const uint32_t e = entry[(v >> 28) & 3u], k = v & 0x0fffffffu;
    return e > k ? e - k : 0u;
}

struct SeqTables {
    const uint32_t* t[3];
    uint32_t log[3];
};
// The sequences' bitstream -> out[0, n_seq]; rep: the three offsets in front (plain, or sym(0..2)) -> behind
SLIMM_ZS_HD inline uint32_t seq_decode(const uint8_t* p, uint64_t len, const SeqTables& t, uint32_t n_seq, uint32_t lit_regen, uint32_t block_max,
                                        Seq* out, uint32_t rep[3], uint32_t& regen) {
    BackBits b;
    if (!b.init(p, len)) return kBadPadding;
    uint32_t sl = b.read(t.log[0]), so = b.read(t.log[1]), sm = b.read(t.log[2]);
    uint32_t lit = 0, pos = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        const uint32_t el = t.t[0][sl], eo = t.t[1][so], em = t.t[2][sm];
        const uint32_t oc = fse_entry_sym(eo);
        if (oc > kOffsetCodeMax) return kBadOffset;
        const uint32_t ofv = (1u << oc) + b.read(oc);
        uint32_t base, bits;
        ml_code(fse_entry_sym(em), base, bits);
        const uint32_t ml = base + b.read(bits);
        ll_code(fse_entry_sym(el), base, bits);
        const uint32_t ll = base + b.read(bits);
        uint32_t off;
        if (ofv > 3u) {
            off = ofv - 3u;
            rep[2] = rep[1], rep[1] = rep[0], rep[0] = off;
        } else {
            const uint32_t idx = ofv - 1u + (ll == 0u ? 1u : 0u);
            if (idx == 0u) off = rep[0];
            else {
                if (idx < 3u) off = rep[idx];
                else if (is_sym(rep[0])) {
                    off = rep[0] + 1u;
                    if ((off & 0x0fffffffu) == 0u) return kBadOffset;
                } else {
                    off = rep[0] - 1u;
                    if (!off) return kBadOffset;
                }
                if (idx > 1u) rep[2] = rep[1];
                rep[1] = rep[0], rep[0] = off;
            }
        }
        out[i].out = pos, out[i].lit = lit, out[i].off = off;
        lit += ll, pos += ll + ml;
        if (lit > lit_regen || pos > block_max) return kBadSequences;
        if (i + 1u < n_seq) {
            sl = fse_entry_base(el) + b.read(fse_entry_bits(el));
            sm = fse_entry_base(em) + b.read(fse_entry_bits(em));
            so = fse_entry_base(eo) + b.read(fse_entry_bits(eo));
        }
    }
    if (b.off != 0) return kBadPadding;
    out[n_seq].out = pos, out[n_seq].lit = lit, out[n_seq].off = 0;
    regen = pos + (lit_regen - lit);
    return regen <= block_max ? kOk : kBlockTooLarge;
}

// ---- XXH64 (seed 0), as a state that takes the text piece by piece
struct Xxh64 {
    static constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull,
                              P5 = 0x27D4EB2F165667C5ull;
    uint64_t v[4], total;
    uint8_t tail[32];
    uint32_t n_tail;
    static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
    static uint64_t round(uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; }
    static uint64_t rd64(const uint8_t* p) {
        uint64_t x;
        memcpy(&x, p, 8);   // (little-endian hosts)
        return x;
    }
    void reset() {
        v[0] = P1 + P2, v[1] = P2, v[2] = 0, v[3] = 0ull - P1;
        total = 0, n_tail = 0;
    }
    void stripe(const uint8_t* p) {
        for (int i = 0; i < 4; ++i) v[i] = round(v[i], rd64(p + 8 * i));
    }
    void update(const uint8_t* p, uint64_t n) {
        total += n;
        if (n_tail) {
            const uint64_t take = n < 32u - n_tail ? n : 32u - n_tail;
            memcpy(tail + n_tail, p, take);
            n_tail += static_cast<uint32_t>(take), p += take, n -= take;
            if (n_tail < 32u) return;
            stripe(tail);
            n_tail = 0;
        }
        for (; n >= 32u; p += 32, n -= 32u) stripe(p);
        if (n) memcpy(tail, p, n);
        n_tail = static_cast<uint32_t>(n);
    }
    uint64_t digest() const {
        uint64_t h;
        if (total >= 32u) {
            h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
            for (int i = 0; i < 4; ++i) h = (h ^ round(0, v[i])) * P1 + P4;
        } else {
            h = P5;
        }
        h += total;
        const uint8_t* p = tail;
        uint32_t n = n_tail;
        for (; n >= 8u; p += 8, n -= 8u) h = rotl(h ^ round(0, rd64(p)), 27) * P1 + P4;
        if (n >= 4u) {
            h = rotl(h ^ (static_cast<uint64_t>(le32(p)) * P1), 23) * P2 + P3;
            p += 4, n -= 4u;
        }
        for (; n; ++p, --n) h = rotl(h ^ (*p * P5), 11) * P1;
        h ^= h >> 33, h *= P2, h ^= h >> 29, h *= P3, h ^= h >> 32;
        return h;
    }
};

// ---- frames and blocks, on the host
// fewer than 4 bytes where a frame may start: the first bytes of a frame's or a skippable frame's magic (the file is cut there)?
inline bool magic_prefix(const uint8_t* p, uint64_t n) {
    const uint8_t m[4] = {0x28, 0xb5, 0x2f, 0xfd}, k[4] = {0x50, 0x2a, 0x4d, 0x18};
    bool frame = true, skip = n > 0 && (p[0] & 0xf0u) == k[0];
    for (uint64_t i = 0; i < n && i < 4u; ++i) {
        frame = frame && p[i] == m[i];
        skip = skip && (i == 0 || p[i] == k[i]);
    }
    return frame || skip;
}
struct FrameHeader {
    uint64_t window, content_size;
    bool has_size, has_checksum;
    uint32_t bytes, block_max;
};
// p at a frame's magic.  kRanOut: more bytes are needed
inline uint32_t frame_header(const uint8_t* p, uint64_t n, FrameHeader& h) {
    if (n < 5u) return kRanOut;
    const uint32_t d = p[4], fcs = d >> 6, single = (d >> 5) & 1u, did = d & 3u;
    if (d & 8u) return kReservedBit;
    const uint32_t did_bytes = did == 3u ? 4u : did, fcs_bytes = fcs == 0u ? single : 1u << fcs;
    h.bytes = 5u + (single ? 0u : 1u) + did_bytes + fcs_bytes;
    if (n < h.bytes) return kRanOut;
    const uint8_t* q = p + 5;
    h.window = 0;
    if (!single) {
        const uint32_t w = *q++;
        const uint64_t wbase = 1ull << (10u + (w >> 3));
        h.window = wbase + (wbase >> 3) * (w & 7u);
    }
    uint32_t dict = 0;
    for (uint32_t i = 0; i < did_bytes; ++i) dict |= static_cast<uint32_t>(*q++) << (8u * i);
    if (dict) return kDictionary;
    h.has_size = fcs_bytes != 0u;
    h.content_size = 0;
    for (uint32_t i = 0; i < fcs_bytes; ++i) h.content_size |= static_cast<uint64_t>(*q++) << (8u * i);
    if (fcs_bytes == 2u) h.content_size += 256u;
    if (single) h.window = h.content_size;
    h.has_checksum = (d & 4u) != 0;
    if (h.window > kWindowMax) return kWindowTooLarge;
    h.block_max = static_cast<uint32_t>(h.window < kBlockMax ? h.window : kBlockMax);
    return kOk;
}

// What a frame's blocks hand on to the ones behind them before any text exists: the descriptions a later block may repeat
struct Entropy {
    bool has_huf = false, has_table[3] = {false, false, false};
    uint8_t huf[kHufDescMax + kPad] = {};
    uint32_t huf_len = 0;
    TableRef kind[3] = {};             // (kind and len; the bytes: desc)
    uint8_t desc[3][160] = {};         // a described table's bytes (at most 53 symbols of at most 10 bits and their zero runs), or the one symbol
    void reset() { *this = Entropy(); }
};

// A compressed block's content at base[at, at + size) -> blk; a table or code that is repeated is copied behind `aux`, which
// the caller keeps in the buffer from aux_base on.  counts (optional): [0] Huffman with a tree, [1] treeless, [2] raw or
// RLE literals, [3..6] tables predefined, one symbol, described, repeated
template <typename Aux>
inline uint32_t plan_compressed(const uint8_t* base, uint64_t at, uint32_t size, Entropy& e, Aux& aux, uint64_t aux_base, Block& blk, uint64_t* counts) {
    const uint8_t* p = base + at;
    LitHeader lh;
    uint32_t st = literals_header(p, size, lh);
    if (st != kOk) return st;
    blk.lit_type = lh.type, blk.lit_regen = lh.regen, blk.lit_streams = lh.streams;
    blk.lit_at = at + lh.bytes, blk.lit_len = lh.comp;
    blk.huf_at = 0, blk.huf_len = 0;
    auto to_aux = [&](const uint8_t* src, uint32_t n) {
        const uint64_t where = aux_base + aux.size();
        aux.insert(aux.end(), src, src + n);
        aux.insert(aux.end(), kPad, uint8_t(0));
        return where;
    };
    if (lh.type == 2u) {
        // (the description's own length: its header byte says)
        if (lh.comp < 1u) return kBadWeights;
        const uint32_t hb = p[lh.bytes], dlen = hb >= 128u ? 1u + (hb - 127u + 1u) / 2u : 1u + hb;
        if (dlen > lh.comp) return kBadWeights;
        blk.huf_at = at + lh.bytes, blk.huf_len = dlen;
        blk.lit_at += dlen, blk.lit_len -= dlen;
        memcpy(e.huf, p + lh.bytes, dlen);
        e.huf_len = dlen, e.has_huf = true;
        if (counts) ++counts[0];
    } else if (lh.type == 3u) {
        if (!e.has_huf) return kNoTable;
        blk.huf_at = to_aux(e.huf, e.huf_len), blk.huf_len = e.huf_len;
        if (counts) ++counts[1];
    } else if (counts) {
        ++counts[2];
    }
    if (lh.type >= 2u && lh.streams == 4u && blk.lit_len < 10u) return kBadLiterals;   // (a jump table and a byte per stream)
    uint64_t q = static_cast<uint64_t>(lh.bytes) + lh.comp;   // the sequences section, in the block
    SeqHeader sh;
    st = sequences_header(p + q, size - q, sh);
    if (st != kOk) return st;
    q += sh.bytes;
    blk.n_seq = sh.n_seq;
    blk.bits_at = 0, blk.bits_len = 0;
    for (uint32_t k = 0; k < 3u; ++k) blk.table[k] = TableRef{kPredefined, 0, 0};
    if (!sh.n_seq) return kOk;
    for (uint32_t k = 0; k < 3u; ++k) {
        TableRef& r = blk.table[k];
        const uint32_t m = sh.mode[k];
        if (counts) ++counts[3u + m];
        if (m == kRepeat) {
            if (!e.has_table[k]) return kNoTable;
            r = e.kind[k];
            if (r.kind != kPredefined) r.at = to_aux(e.desc[k], r.len);
            continue;
        }
        r.kind = m, r.at = at + q, r.len = 0;
        if (m == kRle) {
            if (q >= size) return kBadSequences;
            r.len = 1;
        } else if (m == kFse) {
            int16_t norm[64];
            uint32_t log, n_sym, used = 0;
            st = fse_read_desc(p + q, size - q, k == 1u ? kOFLogMax : k == 0u ? kLLLogMax : kMLLogMax, k == 1u ? kMaxOF : k == 0u ? kMaxLL : kMaxML, norm,
                               log, n_sym, used);
            if (st != kOk) return st;
            if (used > sizeof(e.desc[k])) return kBadFse;
            r.len = used;
        }
        memcpy(e.desc[k], p + q, r.len);
        e.kind[k] = r, e.has_table[k] = true;
        q += r.len;
    }
    if (q >= size) return kBadSequences;
    blk.bits_at = at + q, blk.bits_len = static_cast<uint32_t>(size - q);
    return kOk;
}

// The Huffman literals of a block: the streams' places and byte counts (stream s of 4 gives (regen + 3) / 4 bytes, the last the rest)
struct LitStream {
    uint64_t at;
    uint32_t len, out, count;
};
SLIMM_ZS_HD inline uint32_t literal_streams(const uint8_t* base, const Block& b, LitStream s[4]) {
    if (b.lit_streams == 1u) {
        s[0] = LitStream{b.lit_at, b.lit_len, 0u, b.lit_regen};
        return kOk;
    }
    const uint8_t* j = base + b.lit_at;
    const uint32_t each = (b.lit_regen + 3u) / 4u;
    uint32_t used = 6u, out = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t len = k < 3u ? le16(j + 2u * k) : (b.lit_len >= used ? b.lit_len - used : 0u);
        if (used + len > b.lit_len || !len) return kBadLiterals;
        const uint32_t count = k < 3u ? each : (b.lit_regen >= out ? b.lit_regen - out : 0u);
        if (out + count > b.lit_regen) return kBadLiterals;
        s[k] = LitStream{b.lit_at + used, len, out, count};
        used += len, out += count;
    }
    return kOk;
}

// ---- where a file of frames may be cut (split.hip: slimm_host_zstd_ranges), on the host.  The file is seen through
// read(offset, dst, n) -> bool (false: a read error, or bytes behind `size`): a frame's content is never loaded, only the
// 3 bytes of every block header.
// The block chain from the block header at `at`: every block of a type that exists and no larger than block_max, up to a
// last block, a stated checksum behind it, all within `size`.  *end: the first byte behind the frame
template <typename Read>
inline bool walk_blocks(Read&& read, uint64_t size, uint64_t at, uint32_t block_max, bool has_checksum, uint64_t* end) {
    for (;;) {   // (every turn moves at least 3 bytes on: it ends at `size` at the latest)
        uint8_t b[3];
        if (at > size || size - at < 3u || !read(at, b, 3)) return false;
        const uint32_t h = le24(b), type = (h >> 1) & 3u, len = h >> 3;
        if (type == 3u || len > block_max) return false;
        const uint64_t content = type == kRleBlock ? 1u : len;
        at += 3u;
        if (size - at < content) return false;
        at += content;
        if (h & 1u) break;
    }
    if (has_checksum) {
        if (size - at < 4u) return false;
        at += 4u;
    }
    *end = at;
    return true;
}
// Is `at` the file's end, or do a frame's or a skippable frame's magic bytes stand there?
template <typename Read>
inline bool frame_may_start(Read&& read, uint64_t size, uint64_t at) {
    if (at == size) return true;
    uint8_t m[4];
    if (at > size || size - at < 4u || !read(at, m, 4)) return false;
    const uint32_t magic = le32(m);
    return magic == kMagic || (magic & 0xfffffff0u) == kSkippable;
}
// May the file be cut in front of byte `at`?  A frame starts there whose header parses (frame_header: reserved bit, window,
// dictionary) and whose block chain reaches a last block and a stated checksum inside the file, or a skippable frame
// whose length fits; and behind it the file ends, or the next magic stands.  *end: the first byte behind what starts at `at`
template <typename Read>
inline bool cut_candidate(Read&& read, uint64_t size, uint64_t at, uint64_t* end) {
    uint8_t h[18];   // (a frame header is at most 4 + 1 + 1 + 4 + 8 bytes)
    if (at >= size || size - at < 8u) return false;   // (the smallest frame: magic, descriptor, one empty block)
    const uint64_t n = size - at < sizeof(h) ? size - at : sizeof(h);
    if (!read(at, h, static_cast<size_t>(n))) return false;
    const uint32_t magic = le32(h);
    uint64_t e = 0;
    if ((magic & 0xfffffff0u) == kSkippable) {
        const uint64_t len = le32(h + 4);
        if (size - at - 8u < len) return false;
        e = at + 8u + len;
    } else {
        FrameHeader fh;
        if (magic != kMagic || frame_header(h, n, fh) != kOk) return false;
        if (!walk_blocks(read, size, at + fh.bytes, fh.block_max, fh.has_checksum, &e)) return false;
    }
    if (!frame_may_start(read, size, e)) return false;
    *end = e;
    return true;
}

}  // namespace zs
}  // namespace slimm
