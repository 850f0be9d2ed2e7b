// The zstd container, walked: frames, skippable frames, block headers and checksums as a sequence of items over a span of
// bytes (the format: zstd_frame.h).  ONE walker for the host reader (host/zstd.cpp), which pulls bytes until an item is
// whole, and for the device decoder's round (zstd_decode.hip), which is pushed bytes and waits for them.  Peek, then take:
// peek names what stands at the position and changes nothing, take moves the state past it -- a caller may look at a
// block, leave it for later, and has nothing to undo.  The walker reads no payload: what a block's content decodes to, the
// frame's content size and its checksum's value are the callers' business.  Host only, no HIP.
#pragma once
#include <string>

#include "zstd_frame.h"

namespace slimm {
namespace zs {

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
    enum Kind : uint8_t { More, Error, MayEnd, SkippableFrame, Header, Block, Sum };
    struct Item {
        Kind kind = More;
        Place place = Place::At;
        uint64_t at = 0;            // the place's file offset
        uint32_t status = kOk;
        uint64_t want = 0;
        uint64_t bytes = 0;         // what take() moves past: the caller's position goes on by as much
        FrameHeader fh{};           // Header
        uint32_t type = 0, size = 0;   // Block: its type and stated size; its content is bytes - 3
        bool last = false;
        uint32_t sum = 0;           // Sum: the checksum's value
        std::string where() const { return place_text(place, at); }
        std::string words() const { return where() + ": " + status_text(status); }   // an error in words: "<place> at byte N: <cause>"
        Item& more(uint64_t n, uint32_t verdict = kRanOut) { return kind = More, want = n, status = verdict, *this; }
        Item& error(uint32_t cause) { return kind = Error, status = cause, *this; }
        Item& is(Kind k, uint64_t n) { return kind = k, bytes = n, *this; }
    };

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
            if (magic != kMagic) return it.error(frames ? kNoFrame : kRanOut);
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
        if (avail < 3u) return it.more(3);
        const uint32_t h = le24(p);
        it.type = (h >> 1) & 3u, it.size = h >> 3, it.last = h & 1u;
        it.place = Place::Block;
        if (it.type == 3u) return it.error(kReservedBlock);
        if (it.size > fh.block_max) return it.error(kBlockTooLarge);
        const uint64_t n = 3ull + (it.type == kRleBlock ? 1u : it.size);
        return avail < n ? it.more(n) : it.is(Block, n);
    }

    // past an item that peek has named
    void take(const Item& it) {
        if (it.kind == SkippableFrame) ++frames;
        if (it.kind == Header) fh = it.fh, frame_at = it.at, stage = Blocks, ++frames;
        if (it.kind == Block && it.last) stage = fh.has_checksum ? Checksum : Between;
        if (it.kind == Sum) stage = Between;
    }
};

}  // namespace zs
}  // namespace slimm
