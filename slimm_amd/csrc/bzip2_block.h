// One bzip2 block, decoded: the part of the format both the host reader (host/bzip2.cpp) and the device decoder
// (bzip2_decode.hip) run, the same source for both.  Written from the format as bzip2 writes it:
//   stream  "BZh" + level '1'..'9' (at most level x 100 000 bytes of RLE1 text per block), blocks, end-of-stream marker
//   block   48-bit magic 0x314159265359 (at ANY bit offset: blocks are bit-packed), 32-bit CRC of the block's text,
//           1 "randomised" bit, 24-bit origPtr, the used-byte map (16 + 16 x 16 bits), 2..6 Huffman tables chosen per
//           50 symbols by MTF-coded selectors, code lengths of 1..20 bits (delta-coded), then the symbols: RUNA / RUNB
//           (bijective base-2 run lengths of the front byte), MTF indices, end of block
//   end     48-bit magic 0x177245385090, the combined CRC (c = rotl(c, 1) ^ block CRC over the stream's blocks), padding
//           to a byte; another stream may follow (pbzip2, lbzip2)
// Decoding a block: Huffman -> MTF -> RUNA / RUNB give the BWT string; the inverse BWT from origPtr gives the RLE1 text;
// undoing RLE1 (4 equal bytes + a count byte 0..255) gives the text, whose CRC-32 (MSB first, polynomial 0x04c11db7 --
// not zlib's reflected one) must be the block's.
#pragma once
#include <stdint.h>

#if defined(__host__) && defined(__device__)
#define SLIMM_BZ2_HD __host__ __device__
#else
#define SLIMM_BZ2_HD
#endif

namespace slimm {
namespace bz2 {

constexpr uint64_t kBlockMagic = 0x314159265359ull, kEosMagic = 0x177245385090ull;
constexpr uint32_t kMaxBlock = 900000;      // RLE1 bytes of a level-9 block (the BWT string's length)
constexpr uint32_t kMaxSelectors = 18002;   // what bzip2 writes at most (more are read and dropped, as bzip2 1.0.8 does)
constexpr uint32_t kMaxGroups = 6, kMaxAlpha = 258, kMaxCodeLen = 23;
// A file split by byte range (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE"): a member reads this many bytes behind
// its range, so that the block that starts in the range's last bit can finish there.  From the format's bounds: the
// block's fixed fields (magic 48, CRC 32, randomised 1, origPtr 24, used-byte map 16 + 256, table count 3, selector count
// 15), 2^15 - 1 selectors of at most 6 bits, 6 tables of a 5-bit start and 258 lengths that bzip2 writes in at most 19
// two-bit steps and a stop bit each, kMaxBlock + 1 symbols (every symbol but the end of block gives a byte) of at most 20
// bits, and an end-of-stream marker (magic 48, combined CRC 32, padding 7) with the next stream's header (32); rounded
// up to 64 KiB.  (A table whose lengths wander up and down for longer is not what bzip2 writes: SLIMM_E_SPLIT.)
constexpr uint64_t kSplitSlackBits = (48u + 32u + 1u + 24u + 16u + 256u + 3u + 15u) + 32767ull * 6u + 6ull * (5u + kMaxAlpha * 39ull) +
                                     (kMaxBlock + 1ull) * 20u + (48u + 32u + 7u + 32u);
constexpr uint64_t kSplitSlack = ((kSplitSlackBits + 7u) / 8u + 65535u) & ~65535ull;

// A block's decode status; kRanOut: the bytes at hand end inside the block (more may come)
enum Status : uint32_t {
    kOk = 0,
    kRanOut,
    kRandomised,
    kNoBytesUsed,
    kBadTableCount,
    kBadSelectorCount,
    kBadSelector,
    kBadCodeLength,
    kBadCode,
    kBadRun,
    kTooLong,
    kBadOrigPtr,
    kBadCrc,
    kNoBlock,
    kBadLinks,
    kStatusCount
};
inline const char* status_text(uint32_t s) {
    static const char* const t[kStatusCount] = {"ok",
                                                "truncated",
                                                "randomised block (bzip2 before 0.9.5): refused",
                                                "no byte value in use",
                                                "bad number of Huffman tables",
                                                "bad number of selectors",
                                                "selector past the Huffman tables",
                                                "bad Huffman code length",
                                                "bad Huffman code",
                                                "bad run length",
                                                "block longer than its stream's level allows",
                                                "origPtr out of range",
                                                "block CRC mismatch",
                                                "no block or end-of-stream magic",
                                                "inverse BWT links inconsistent"};
    return s < kStatusCount ? t[s] : "unknown error";
}

// MSB-first bit reader over bytes[0, end_bit / 8): at most 32 bits a call
struct Bits {
    const uint8_t* p;
    uint64_t next, end;   // next byte to load, bytes at hand
    uint64_t acc;         // n bits not handed out yet, at the low end
    uint32_t n;
    SLIMM_BZ2_HD Bits(const uint8_t* bytes, uint64_t bit, uint64_t end_bit) : p(bytes), next(bit >> 3), end(end_bit >> 3), acc(0), n(0) {
        uint32_t drop = static_cast<uint32_t>(bit & 7u), v;
        if (drop) (void)get(drop, v);
    }
    SLIMM_BZ2_HD uint64_t pos() const { return next * 8u - n; }
    SLIMM_BZ2_HD bool get(uint32_t k, uint32_t& v) {
        while (n < k) {
            if (next >= end) return false;
            acc = (acc << 8) | p[next++];
            n += 8;
        }
        n -= k;
        v = static_cast<uint32_t>((acc >> n) & ((1ull << k) - 1u));
        return true;
    }
    SLIMM_BZ2_HD bool peek48(uint64_t& v) {   // the next 48 bits, not consumed
        uint32_t hi, lo;
        const uint64_t a = acc, nx = next;
        const uint32_t nn = n;
        if (!get(24, hi) || !get(24, lo)) {
            acc = a, next = nx, n = nn;
            return false;
        }
        acc = a, next = nx, n = nn;
        v = (static_cast<uint64_t>(hi) << 24) | lo;
        return true;
    }
};

// What decoding a block's symbols found
struct BlockInfo {
    uint32_t status;
    uint32_t crc;        // the CRC the block carries
    uint32_t orig_ptr;
    uint32_t n;          // BWT string length
    uint64_t end_bit;    // first bit behind the block (valid when status == kOk)
};

// Scratch of one block's decode (about 27 KB: LDS on the device)
struct Tables {
    int32_t limit[kMaxGroups][kMaxCodeLen];
    int32_t base[kMaxGroups][kMaxCodeLen];
    int32_t perm[kMaxGroups][kMaxAlpha];
    int32_t min_len[kMaxGroups];
    uint8_t len[kMaxGroups][kMaxAlpha];
    uint8_t selector[kMaxSelectors];
    uint8_t seq_to_unseq[256];
    uint8_t mtf[256];
};

// The block whose 48-bit magic starts at bit `bit` (the magic is not checked here: the caller found it): its symbols decoded
// into the BWT string ll[0, n) (room for max_n bytes) and counts[256] (its byte histogram).  bytes[0, end_bit/8) are at
// hand.  Returns the status, info filled.
SLIMM_BZ2_HD inline uint32_t decode_block(const uint8_t* bytes, uint64_t bit, uint64_t end_bit, uint32_t max_n, Tables& t, uint8_t* ll,
                                          uint32_t* counts, BlockInfo& info) {
    info.status = kRanOut;
    info.crc = info.orig_ptr = info.n = 0;
    info.end_bit = 0;
    Bits in(bytes, bit + 48u, end_bit);
    uint32_t v, crc_hi, crc_lo;
#define SLIMM_BZ2_GET(k, out)               \
    do {                                    \
        if (!in.get((k), (out))) return info.status = kRanOut; \
    } while (0)
    if (bit + 48u > end_bit) return info.status = kRanOut;
    SLIMM_BZ2_GET(16, crc_hi);
    SLIMM_BZ2_GET(16, crc_lo);
    info.crc = (crc_hi << 16) | crc_lo;
    SLIMM_BZ2_GET(1, v);
    if (v) return info.status = kRandomised;
    SLIMM_BZ2_GET(24, info.orig_ptr);
    // the used-byte map
    uint32_t in_use16, n_in_use = 0;
    SLIMM_BZ2_GET(16, in_use16);
    for (uint32_t i = 0; i < 16; ++i) {
        if (!(in_use16 & (0x8000u >> i))) continue;
        uint32_t w;
        SLIMM_BZ2_GET(16, w);
        for (uint32_t j = 0; j < 16; ++j)
            if (w & (0x8000u >> j)) t.seq_to_unseq[n_in_use++] = static_cast<uint8_t>(i * 16u + j);
    }
    if (n_in_use == 0) return info.status = kNoBytesUsed;
    const uint32_t alpha = n_in_use + 2u;
    uint32_t n_groups, n_sel;
    SLIMM_BZ2_GET(3, n_groups);
    if (n_groups < 2 || n_groups > kMaxGroups) return info.status = kBadTableCount;
    SLIMM_BZ2_GET(15, n_sel);
    if (n_sel < 1) return info.status = kBadSelectorCount;
    // the selectors, MTF-coded (unary), undone at once
    uint8_t pos[kMaxGroups];
    for (uint32_t g = 0; g < n_groups; ++g) pos[g] = static_cast<uint8_t>(g);
    for (uint32_t i = 0; i < n_sel; ++i) {
        uint32_t j = 0;
        for (;;) {
            SLIMM_BZ2_GET(1, v);
            if (!v) break;
            if (++j >= n_groups) return info.status = kBadSelector;
        }
        const uint8_t s = pos[j];
        for (; j > 0; --j) pos[j] = pos[j - 1];
        pos[0] = s;
        if (i < kMaxSelectors) t.selector[i] = s;
    }
    if (n_sel > kMaxSelectors) n_sel = kMaxSelectors;
    // the code lengths, delta-coded, and the canonical decode tables (limit / base / perm per code length)
    for (uint32_t g = 0; g < n_groups; ++g) {
        uint32_t cur;
        SLIMM_BZ2_GET(5, cur);
        int32_t mn = 32, mx = 0;
        for (uint32_t i = 0; i < alpha; ++i) {
            for (;;) {
                if (cur < 1 || cur > 20) return info.status = kBadCodeLength;
                SLIMM_BZ2_GET(1, v);
                if (!v) break;
                SLIMM_BZ2_GET(1, v);
                cur = v ? cur - 1u : cur + 1u;
            }
            t.len[g][i] = static_cast<uint8_t>(cur);
            mn = static_cast<int32_t>(cur) < mn ? static_cast<int32_t>(cur) : mn;
            mx = static_cast<int32_t>(cur) > mx ? static_cast<int32_t>(cur) : mx;
        }
        int32_t* limit = t.limit[g];
        int32_t* base = t.base[g];
        int32_t* perm = t.perm[g];
        int32_t pp = 0;
        for (int32_t l = mn; l <= mx; ++l)
            for (uint32_t i = 0; i < alpha; ++i)
                if (t.len[g][i] == l) perm[pp++] = static_cast<int32_t>(i);
        for (uint32_t i = 0; i < kMaxCodeLen; ++i) base[i] = limit[i] = 0;
        for (uint32_t i = 0; i < alpha; ++i) base[t.len[g][i] + 1]++;
        for (uint32_t i = 1; i < kMaxCodeLen; ++i) base[i] += base[i - 1];
        int32_t vec = 0;
        for (int32_t l = mn; l <= mx; ++l) {
            vec += base[l + 1] - base[l];
            limit[l] = vec - 1;
            vec <<= 1;
        }
        for (int32_t l = mn + 1; l <= mx; ++l) base[l] = ((limit[l - 1] + 1) << 1) - base[l];
        t.min_len[g] = mn;
    }
    // the symbols
    for (uint32_t i = 0; i < 256; ++i) {
        t.mtf[i] = static_cast<uint8_t>(i);
        counts[i] = 0;
    }
    const uint32_t eob = n_in_use + 1u;
    uint32_t group = 0, group_left = 0, nblock = 0;
    const int32_t* limit = nullptr;
    const int32_t* base = nullptr;
    const int32_t* perm = nullptr;
    int32_t min_len = 0;
    uint32_t run = 0, run_w = 1;   // a RUNA / RUNB run being summed: its length so far, the next digit's weight
    for (;;) {
        if (group_left == 0) {
            if (group >= n_sel) return info.status = kBadSelector;
            const uint32_t g = t.selector[group++];
            limit = t.limit[g];
            base = t.base[g];
            perm = t.perm[g];
            min_len = t.min_len[g];
            group_left = 50;
        }
        --group_left;
        int32_t zn = min_len;
        uint32_t zv;
        SLIMM_BZ2_GET(static_cast<uint32_t>(zn), zv);
        int32_t zvec = static_cast<int32_t>(zv);
        while (zvec > limit[zn]) {
            if (++zn > 20) return info.status = kBadCode;
            SLIMM_BZ2_GET(1, v);
            zvec = (zvec << 1) | static_cast<int32_t>(v);
        }
        const int32_t idx = zvec - base[zn];
        if (idx < 0 || idx >= static_cast<int32_t>(alpha)) return info.status = kBadCode;
        const uint32_t sym = static_cast<uint32_t>(perm[idx]);
        if (sym <= 1u) {   // RUNA (1 x weight) / RUNB (2 x weight)
            run += run_w << sym;
            run_w <<= 1;
            if (run_w >= (2u << 20)) return info.status = kBadRun;
            continue;
        }
        if (run) {   // a run ends: the front byte, `run` times
            const uint8_t b = t.seq_to_unseq[t.mtf[0]];
            if (run > max_n - nblock) return info.status = kTooLong;
            counts[b] += run;
            for (uint32_t k = 0; k < run; ++k) ll[nblock++] = b;
            run = 0;
            run_w = 1;
        }
        if (sym == eob) break;
        if (nblock >= max_n) return info.status = kTooLong;
        uint32_t nn = sym - 1u;
        const uint8_t u = t.mtf[nn];
        for (; nn > 0; --nn) t.mtf[nn] = t.mtf[nn - 1];
        t.mtf[0] = u;
        const uint8_t b = t.seq_to_unseq[u];
        counts[b]++;
        ll[nblock++] = b;
    }
#undef SLIMM_BZ2_GET
    info.n = nblock;
    info.end_bit = in.pos();
    if (info.orig_ptr >= nblock) return info.status = kBadOrigPtr;
    return info.status = kOk;
}

// Inverse BWT, step 1 (a counting sort of the BWT string, stores only): link[j] = {the position i that follows sorted
// position j | ll[i] << 24}.  The text (RLE1 bytes) is then n steps from p = origPtr: u = link[p], byte u >> 24,
// p = u & 0xffffff.  (A text that is one string repeated d times gives d cycles of n / d links: the n steps go round the
// cycle through origPtr d times, as bzip2's own decoder does.)  cf: 256 words of scratch (LDS on the device)
SLIMM_BZ2_HD inline void link_block(const uint8_t* ll, uint32_t n, const uint32_t* counts, uint32_t* link, uint32_t* cf) {
    uint32_t s = 0;
    for (uint32_t i = 0; i < 256; ++i) {
        cf[i] = s;
        s += counts[i];
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = ll[i];
        link[cf[b]++] = i | (b << 24);
    }
}
constexpr uint32_t kLinkMask = 0xffffffu;

// RLE1 undone: the state between bytes (the byte of the run, its length 1..4, 0 = none; after 4 the next byte is a count)
struct Rle1 {
    uint32_t last = 256u, run = 0;
    // `b` -> *copies of *out (0: a count byte of 0)
    SLIMM_BZ2_HD uint32_t step(uint32_t b, uint32_t& out) {
        if (run == 4u) {
            run = 0;
            out = last;
            last = 256u;
            return b;
        }
        if (b == last) {
            ++run;
        } else {
            last = b;
            run = 1;
        }
        out = b;
        return 1u;
    }
    // behind a block's last byte: four equal bytes stand there and their count byte is missing.  bzip2 itself refuses such
    // a block (its reader runs past the block's end); so does every user of this struct, in the words of kBadRun
    SLIMM_BZ2_HD bool count_missing() const { return run == 4u; }
};
constexpr uint32_t kLenBadLinks = ~0u, kLenBadRun = ~0u - 1u;   // k_bz2_unbwt's text_len of a block it refuses
constexpr uint64_t kNoTextLength = ~0ull;

// the length of a block's text (RLE1 undone) from its links: the n-step walk without the bytes (the host's planner of
// slimm_host_bzip2_ranges counts decoded bytes up to the SAM header's end); kNoTextLength: the last run's count byte is missing
inline uint64_t text_length(const uint32_t* link, uint32_t n, uint32_t orig_ptr) {
    Rle1 st;
    uint64_t len = 0;
    uint32_t p = orig_ptr, byte;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t u = link[p];
        len += st.step(u >> 24, byte);
        p = u & kLinkMask;
    }
    return st.count_missing() ? kNoTextLength : len;
}

SLIMM_BZ2_HD inline void crc_table(uint32_t* tab) {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : (c << 1);
        tab[i] = c;
    }
}
SLIMM_BZ2_HD inline uint32_t crc_byte(const uint32_t* tab, uint32_t crc, uint32_t b) { return (crc << 8) ^ tab[(crc >> 24) ^ b]; }

}  // namespace bz2
}  // namespace slimm
