// The .xz container, walked: stream padding, stream headers, block headers, LZMA2 chunk headers, block ends, indexes and
// footers as a sequence of items over a span of bytes (the format: xz_stream.h).  ONE walker for the host reader
// (host/xz.cpp), which pulls bytes until an item is whole and decodes chunk by chunk, and for the device decoder's round
// (xz_decode.hip), which is pushed bytes and takes whole blocks.  Peek, then take: peek names what stands at the position
// and changes nothing, take moves the state past it.  The state inside a block (`block`) is plain data: a caller that finds
// a block's bytes not all at hand puts it back by value (leave_block); the stream's records grow only at a block's end.
// The walker decodes no chunk and compares no check field.  Host only, no HIP.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "xz_stream.h"

namespace slimm {
namespace xz {

// where in the file something stood: what an error names
enum class Place : uint8_t { At, StreamHeader, BlockHeader, Block, Chunk, Index, Footer };
inline std::string place_text(Place w, uint64_t at) {
    static const char* const t[] = {"at", "stream header at", "block header at", "block at", "chunk at", "index at", "stream footer at"};
    return std::string(t[static_cast<uint32_t>(w)]) + " byte " + std::to_string(at);
}
inline bool all_zero(const uint8_t* p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

struct Walker {
    using Record = std::pair<uint64_t, uint64_t>;   // a block as its stream's index states it: unpadded size, uncompressed size
    enum Stage : uint8_t { Between, Blocks, Chunks } stage = Between;   // between streams, among a stream's blocks, among a block's chunks
    uint32_t check = 0;             // the stream's check kind
    uint64_t streams = 0;           // streams so far
    std::vector<Record> records;    // the stream's blocks so far
    // a walk that starts among the blocks of a stream whose header it has not seen (among_blocks): until that stream's
    // index, `records` holds only the blocks met, and the index's records in front of those cannot be checked
    bool open_left = false;
    struct InBlock {   // the block at hand: where its header starts, the header, its compressed and text bytes so far, the chunk rules
        uint64_t at = 0;
        BlockHeader bh{};
        uint64_t comp = 0, text = 0;
        Rules rules;
    } block;

    // More: the bytes end inside what stands here -- `want` of them are needed at least, and `place` and `status` are the
    // verdict if the input is over.  Error: `status`.  MayEnd: no byte is left, and the streams may end here
    enum Kind : uint8_t { More, Error, MayEnd, Padding, StreamStart, BlockStart, ChunkItem, BlockEnd, Index };
    struct Item {
        Kind kind = More;
        Place place = Place::At;
        uint64_t at = 0;            // the place's file offset
        uint32_t status = kOk;
        uint64_t want = 0;
        uint64_t bytes = 0;         // what take() moves past: the caller's position goes on by as much
        uint32_t check = 0;         // StreamStart: its check kind
        BlockHeader bh{};           // BlockStart: the header (an error of kBadFilter: its filter_id)
        Chunk chunk{};              // ChunkItem: the header; the chunk's bytes are chunk.header + chunk.csize
        Rules rules;                // ... and the rules behind it
        uint32_t pad = 0;           // BlockEnd: the end marker, `pad` zero bytes, the check field
        Record record{};            // ... and the record it appends
        uint64_t count = 0, index_bytes = 0;   // Index: its records and bytes; the footer lies behind them
        std::vector<Record> kept;   // ... and the leading records that could not be checked (open_left)
        std::string where() const { return place_text(place, at); }
        Item& more(uint64_t n, uint32_t verdict = kRanOut) { return kind = More, want = n, status = verdict, *this; }
        Item& error(uint32_t cause) { return kind = Error, status = cause, *this; }
        Item& is(Kind k, uint64_t n) { return kind = k, bytes = n, *this; }
        // an error in words: "<place> at byte N: <cause>"
        std::string words() const {
            return where() + ": " + status_text(status) + (status == kBadFilter ? " (filter id " + std::to_string(bh.filter_id) + ")" : "");
        }
    };

    // the state that being told the stream's check kind gives: the walk starts at a block's first byte
    void among_blocks(uint32_t told_check) { stage = Blocks, check = told_check, streams = 1, open_left = true; }
    // back in front of the block whose header was taken: `saved` is `block` as it was then
    void leave_block(const InBlock& saved) { stage = Blocks, block = saved; }

    // what stands at p[0, avail), file offset `base`
    Item peek(const uint8_t* p, uint64_t avail, uint64_t base) const {
        Item it;
        it.at = base;
        if (stage == Between) {
            if (streams > 0 && avail >= 4u && all_zero(p, 4)) return it.is(Padding, 4);
            if (avail == 0 && streams > 0) return it.is(MayEnd, 0);
            if (avail < kHeaderBytes) {   // (a file that ends inside a magic is truncated; else: what the bytes are not)
                if (streams == 0 || magic_prefix(p, avail)) return it.place = Place::StreamHeader, it.more(kHeaderBytes);
                return it.more(kHeaderBytes, all_zero(p, avail) ? kBadPadding : kTrailing);
            }
            if (!is_magic(p)) return it.error(streams > 0 && p[0] == 0 ? kBadPadding : kTrailing);
            it.place = Place::StreamHeader;
            const uint32_t st = stream_header(p, &it.check);
            return st != kOk ? it.error(st) : it.is(StreamStart, kHeaderBytes);
        }
        if (stage == Blocks && avail >= 1u && p[0] == 0) return peek_index(p, avail, it);
        if (stage == Blocks) {
            it.place = Place::BlockHeader;
            const uint32_t st = block_header(p, avail, it.bh);
            if (st == kRanOut) return it.more(avail + 1u);
            return st != kOk ? it.error(st) : it.is(BlockStart, it.bh.bytes);
        }
        it.place = Place::Chunk;
        it.rules = block.rules;
        const uint32_t st = chunk_header(p, avail, it.rules, it.chunk);
        if (st == kRanOut) return it.more(avail + 1u);
        if (st != kOk) return it.error(st);
        if (it.chunk.control != 0) {
            const uint64_t n = static_cast<uint64_t>(it.chunk.header) + it.chunk.csize;
            return avail < n ? it.more(n) : it.is(ChunkItem, n);
        }
        // the end marker: the padding behind it, the sizes against the header's, the check field's room
        it.place = Place::Block, it.at = block.at;
        const uint64_t comp = block.comp + 1u, cb = check_bytes(check);
        it.pad = static_cast<uint32_t>((4u - ((block.bh.bytes + comp) & 3u)) & 3u);
        if (avail < 1u + it.pad + cb) return it.more(1u + it.pad + cb);
        if (!all_zero(p + 1, it.pad)) return it.error(kBadBlockPadding);
        if ((block.bh.has_compressed && block.bh.compressed != comp) || (block.bh.has_uncompressed && block.bh.uncompressed != block.text))
            return it.error(kBadBlockSizes);
        it.record = Record(block.bh.bytes + comp + cb, block.text);
        return it.is(BlockEnd, 1u + it.pad + cb);
    }

    // past an item that peek has named
    void take(const Item& it) {
        if (it.kind == StreamStart) check = it.check, records.clear(), ++streams, stage = Blocks;
        if (it.kind == BlockStart) block = InBlock{it.at, it.bh, 0, 0, Rules{}}, stage = Chunks;
        if (it.kind == ChunkItem) block.rules = it.rules, block.comp += it.bytes, block.text += it.chunk.usize;
        if (it.kind == BlockEnd) records.push_back(it.record), stage = Blocks;
        if (it.kind == Index) records.clear(), open_left = false, stage = Between;
    }

private:
    // the index held record by record against the blocks met, and the footer behind it with its backward size
    Item peek_index(const uint8_t* p, uint64_t avail, Item& it) const {
        it.place = Place::Index;
        uint64_t at = 0;
        const uint32_t st = index_extent(p, avail, &it.count, &at, &it.index_bytes);
        if (st == kRanOut) return it.more(avail + 1u);
        if (st != kOk) return it.error(st);
        if (open_left ? it.count < records.size() : it.count != records.size()) return it.error(kIndexMismatch);
        Record r;
        for (uint64_t k = it.count - records.size(); k; --k) {
            index_record(p, it.index_bytes, &at, &r.first, &r.second);
            it.kept.push_back(r);
        }
        for (const Record& mine : records) {
            index_record(p, it.index_bytes, &at, &r.first, &r.second);
            if (r != mine) return it.error(kIndexMismatch);
        }
        it.place = Place::Footer, it.at += it.index_bytes;
        if (avail < it.index_bytes + kHeaderBytes) return it.more(it.index_bytes + kHeaderBytes);
        uint64_t stated = 0;
        uint32_t fs = stream_footer(p + it.index_bytes, check, &stated);
        if (fs == kOk && stated != it.index_bytes) fs = kBadFooter;
        if (fs != kOk) return it.error(fs);
        return it.is(Index, it.index_bytes + kHeaderBytes);
    }
};

}  // namespace xz
}  // namespace slimm
