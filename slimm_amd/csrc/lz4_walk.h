// The LZ4 container, walked: frames, skippable frames, block headers, end marks and checksums as a sequence of items over a
// span of bytes (the format: lz4_frame.h).  ONE walker for the host reader (host/lz4.cpp), which pulls bytes until an item
// is whole, and for the device decoder's round (lz4_decode.hip), which is pushed bytes and waits for them -- as zs::Walker
// is (zstd_walk.h).  Peek, then take: peek names what stands at the position and changes nothing, take moves the state past
// it.  The walker reads no payload: what a block decodes to, whether its checksum holds, the frame's content size and its
// checksum's value are the callers' business.  Host only, no HIP.
#pragma once
#include <string>

#include "lz4_frame.h"

namespace slimm {
namespace lz4 {

// where in the file something stood: what an error names
enum class Place : uint8_t { At, FrameHeader, Skippable, BlockHeader, Block, Checksum, Frame };
inline std::string place_text(Place w, uint64_t at) {
    static const char* const t[] = {"at", "frame header at", "skippable frame at", "block header at", "block at", "checksum at", "frame at"};
    return std::string(t[static_cast<uint32_t>(w)]) + " byte " + std::to_string(at);
}

struct Walker {
    enum Stage : uint8_t { Between, Blocks, Checksum } stage = Between;   // between frames, among a frame's blocks, at its checksum
    FrameHeader fh{};       // of the frame at hand
    uint64_t frame_at = 0;  // ... and its file offset
    uint64_t frames = 0;    // frames so far, skippable ones too

    // More: the bytes end inside what stands here -- `want` of them are needed at least, and `status` is the verdict if the
    // input is over.  Error: `status`.  MayEnd: no byte is left, and the frames may end here
    enum Kind : uint8_t { More, Error, MayEnd, SkippableFrame, Header, Block, EndMark, Sum };
    struct Item {
        Kind kind = More;
        Place place = Place::At;
        uint64_t at = 0;            // the place's file offset
        uint32_t status = kOk;
        uint64_t want = 0;
        uint64_t bytes = 0;         // what take() moves past: the caller's position goes on by as much
        FrameHeader fh{};           // Header
        uint32_t size = 0;          // Block: its bytes, which lie 4 bytes behind the item's first
        bool stored = false;
        uint32_t sum = 0;           // Block: its checksum where the frame has them; Sum: the content checksum
        std::string where() const { return place_text(place, at); }
        std::string words() const { return where() + ": " + status_text(status); }   // an error in words: "<place> at byte N: <cause>"
        Item& more(uint64_t n, uint32_t verdict = kRanOut) { return kind = More, want = n, status = verdict, *this; }
        Item& error(uint32_t cause) { return kind = Error, status = cause, *this; }
        Item& is(Kind k, uint64_t n) { return kind = k, bytes = n, *this; }
    };

    static bool magic_prefix(const uint8_t* p, uint64_t n) {   // the first n < 4 bytes of a frame's or a skippable frame's magic
        static const uint8_t frame[4] = {0x04, 0x22, 0x4d, 0x18};
        bool a = true, b = true;
        for (uint64_t i = 0; i < n; ++i) a = a && p[i] == frame[i], b = b && (i == 0 ? (p[0] & 0xf0u) == 0x50u : p[i] == (i == 1 ? 0x2au : 0x4du));
        return a || b;
    }

    // what stands at p[0, avail), file offset `base`
    Item peek(const uint8_t* p, uint64_t avail, uint64_t base) const {
        Item it;
        it.at = base;
        if (stage == Between) {
            if (avail == 0 && frames > 0) return it.is(MayEnd, 0);
            // (a file that ends inside a magic is truncated, one that ends in other bytes behind its frames holds no frame there)
            if (avail < 4u) return it.more(4, frames == 0 || magic_prefix(p, avail) ? kRanOut : kNoFrame);
            const uint32_t magic = le32(p);
            if ((magic & 0xfffffff0u) == kSkippable) {
                it.place = Place::Skippable;
                if (avail < 8u) return it.more(8);
                const uint64_t n = 8ull + le32(p + 4);
                return avail < n ? it.more(n) : it.is(SkippableFrame, n);
            }
            it.place = Place::FrameHeader;
            if (magic == kLegacyMagic) return it.error(kLegacy);
            it.place = Place::At;
            if (magic != kMagic) return it.error(frames ? kNoFrame : kNotLz4);
            it.place = Place::FrameHeader;
            const uint32_t st = frame_header(p, avail, it.fh);
            if (st == kRanOut) return it.more(avail + 1u);
            return st != kOk ? it.error(st) : it.is(Header, it.fh.bytes);
        }
        if (stage == Checksum) {
            it.place = Place::Checksum;
            if (avail < 4u) return it.more(4);
            it.sum = le32(p);
            return it.is(Sum, 4);
        }
        it.place = Place::BlockHeader;
        if (avail < 4u) return it.more(4);
        const uint32_t h = le32(p);
        if (!h) return it.is(EndMark, 4);
        it.stored = (h >> 31) != 0, it.size = h & 0x7fffffffu;
        it.place = Place::Block;
        if (it.size > fh.block_max) return it.error(kBlockTooLarge);
        const uint64_t n = 4ull + it.size + (fh.block_sums ? 4u : 0u);
        if (avail < n) return it.more(n);
        if (fh.block_sums) it.sum = le32(p + 4u + it.size);
        return it.is(Block, n);
    }

    // past an item that peek has named
    void take(const Item& it) {
        if (it.kind == SkippableFrame) ++frames;
        if (it.kind == Header) fh = it.fh, frame_at = it.at, stage = Blocks, ++frames;
        if (it.kind == EndMark) stage = fh.has_checksum ? Checksum : Between;
        if (it.kind == Sum) stage = Between;
    }
};

}  // namespace lz4
}  // namespace slimm
