// One file -- BAM, SAM text, BGZF blocks of SAM text, bzip2 SAM, zstd SAM or xz SAM -- split by byte range over a group's members
// (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE"): the host's plan of the ranges (slimm_host_bgzf_ranges,
// slimm_host_text_ranges, slimm_host_bzip2_ranges, slimm_host_zstd_ranges, slimm_host_xz_ranges) and the per-member steps of slimm_group_stitch_ranges (split.h; group.hip runs them cut by cut).  A range that starts inside
// the file guesses its first record as k_bam_pieces guesses a piece's (windows.hip, bam_decode.hip: k_bam_first_guess);
// the member on its left confirms the guess one level up, as k_bam_verify confirms a piece's: its incomplete last record
// followed by the right member's head must be whole records that end exactly where the guess begins.  A range of SAM
// text guesses nothing: its first line starts behind its first newline (sam_decode.hip: k_sam_first_newline), and the
// left member's last line must end with the head.  A range of bzip2 SAM starts at the first block of its own
// (bzip2_decode.hip) and is text from there on; its chain of blocks is held against its neighbours' first (split_bz2_chains).  A range of zstd SAM starts and ends where frames do
// (zstd_decode.hip) and is text in between; that every member's frames ended at its range's end is checked first (split_zstd_ends).  A range of xz SAM starts at a stream header or at a block and ends where
// a block or a stream does (xz_decode.hip); the blocks of a stream that lies over cuts are held against its index (split_xz_streams).  The reference reads one file with one reader (src/misc.hpp:498-522).
#include "context.h"
#include "split.h"
#include "split_plan.h"
#include "gzip_plan.h"
#include "host/zstd.cpp"   // (the host's serial zstd decoder, for the header's frames: the library holds no other copy of it)
#include "host/xz.cpp"     // (xz_read_index and the planner on it: the same)

namespace {

inline uint32_t rd16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8); }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// the BGZF header at h (18 bytes): the block's size (BSIZE + 1), 0 when h is none -- gzip magic, deflate, FEXTRA, XLEN = 6,
// one BC subfield of two bytes (SAM specification 4.1), and room for the 8-byte trailer and an empty deflate stream
uint32_t bgzf_header_size(const uint8_t* h) {
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return 0;
    if (rd16(h + 10) != 6 || h[12] != 'B' || h[13] != 'C' || rd16(h + 14) != 2) return 0;
    const uint32_t total = rd16(h + 16) + 1u;
    return total >= 28u ? total : 0u;
}

struct BgzfFile : slimm::PlanFile {   // (where blocks start)
    uint32_t header_at(uint64_t off) const {   // the block size of a header at off, 0 when there is none
        uint8_t h[18];
        if (off + 18 > size || !read(off, h, 18)) return 0;
        const uint32_t total = bgzf_header_size(h);
        return (total && off + total <= size) ? total : 0u;
    }
    // a block starts at p: its header and the next three chain through BSIZE + 1, or the chain reaches the EOF block
    // (28 bytes, ISIZE 0) or the file's end.  (Compressed bytes may hold a header look-alike; a chain of them hardly.)
    bool chain_at(uint64_t p) const {
        uint64_t off = p;
        for (int k = 0; k < 4; ++k) {
            if (k && off == size) return true;
            const uint32_t total = header_at(off);
            if (!total) return false;
            if (k && total == 28u) {
                uint8_t t[4];
                if (read(off + 24, t, 4) && rd32(t) == 0) return true;
            }
            off += total;
        }
        return true;
    }
    // the first block start at or behind t (the file's size when there is none)
    uint64_t cut_at(uint64_t t) const {
        std::vector<uint8_t> buf(1u << 20);
        while (t + 18 <= size) {
            const size_t n = static_cast<size_t>(std::min<uint64_t>(buf.size(), size - t));
            if (!read(t, buf.data(), n)) return size;
            for (size_t i = 0; i + 18 <= n; ++i)
                if (buf[i] == 0x1f && buf[i + 1] == 0x8b && bgzf_header_size(&buf[i]) && chain_at(t + i)) return t + i;
            t += n - 17;
        }
        return size;
    }
};

}  // namespace

extern "C" {

uint64_t slimm_record_cap(void) { return slimm::record_cap(); }

int slimm_host_bgzf_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    if (!path || !n || !offsets_out) return SLIMM_E_INVALID;
    BgzfFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    // no cut in front of the first block whose inflated bytes start at or behind `skip`: member 0 holds the whole header
    uint64_t floor = 0, before = 0;
    while (skip && before < skip && floor < f.size) {
        const uint32_t total = f.header_at(floor);
        uint8_t t[4];
        if (!total || !f.read(floor + total - 4, t, 4)) return SLIMM_E_INVALID;   // (not a BGZF file)
        before += rd32(t);
        floor += total;
    }
    slimm::even_ranges(floor, f.size, n, offsets_out, [&](uint64_t t) { return f.cut_at(t); });
    return SLIMM_OK;
}

// plain text is cut anywhere: the device finds the line starts (windows.hip: guess_first_record)
int slimm_host_text_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    if (!path || !n || !offsets_out) return SLIMM_E_INVALID;
    uint64_t size = 0;
    if (!slimm::PlanFile::regular_size(path, &size) || skip > size) return SLIMM_E_INVALID;   // (the file is not opened)
    slimm::even_ranges(skip, size, n, offsets_out, [](uint64_t t) { return t; });
    offsets_out[0] = skip;   // (member 0 reads from the first alignment line on)
    return SLIMM_OK;
}

uint64_t slimm_bzip2_split_slack(void) { return slimm::bz2::kSplitSlack; }

// bzip2 is cut at plain byte offsets: a block belongs to the range its magic's first bit lies in, and the device finds the
// blocks (bzip2_decode.hip).  Only the SAM header is decoded here, block by block from the file's start, for the floor
int slimm_host_bzip2_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    namespace bz2 = slimm::bz2;
    if (!path || !n || !offsets_out) return SLIMM_E_INVALID;
    slimm::PlanFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    std::vector<uint8_t> in;
    auto more = [&]() {   // the file's next bytes behind `in` (false: none left, or a read error)
        const size_t have = in.size(), add = static_cast<size_t>(std::min<uint64_t>(f.size - have, std::max<uint64_t>(4u << 20, have)));
        if (!add) return false;
        in.resize(have + add);
        return f.read(have, in.data() + have, add);
    };
    if (!more() || in.size() < 4 || memcmp(in.data(), "BZh", 3) != 0 || in[3] < '1' || in[3] > '9') return SLIMM_E_INVALID;
    // no cut in front of the end of the block that holds decoded byte skip - 1: member 0 holds the whole header
    uint64_t bit = 0, decoded = 0;
    bool in_stream = false;
    std::unique_ptr<bz2::Tables> t(new bz2::Tables);
    std::vector<uint8_t> ll;
    std::vector<uint32_t> link, counts(256), cf(256);
    while (decoded < skip) {
        if (!in_stream) {
            const uint64_t at = bit >> 3;
            if (at + 4 > in.size()) {
                if (!more()) return SLIMM_E_INVALID;   // (the streams end in front of decoded byte `skip`)
                continue;
            }
            if (memcmp(in.data() + at, "BZh", 3) != 0 || in[at + 3] < '1' || in[at + 3] > '9') return SLIMM_E_INVALID;
            in_stream = true;
            bit += 32;
        }
        bz2::Bits br(in.data(), bit, in.size() * 8u);
        uint64_t magic;
        uint32_t v;
        if (!br.peek48(magic)) {
            if (!more()) return SLIMM_E_INVALID;
            continue;
        }
        if (magic == bz2::kEosMagic) {
            if (!br.get(24, v) || !br.get(24, v) || !br.get(16, v) || !br.get(16, v)) {
                if (!more()) return SLIMM_E_INVALID;
                continue;
            }
            bit = (br.pos() + 7u) & ~7ull;
            in_stream = false;
            continue;
        }
        if (magic != bz2::kBlockMagic) return SLIMM_E_INVALID;
        ll.resize(bz2::kMaxBlock);
        link.resize(bz2::kMaxBlock);
        bz2::BlockInfo info;
        const uint32_t status = bz2::decode_block(in.data(), bit, in.size() * 8u, bz2::kMaxBlock, *t, ll.data(), counts.data(), info);
        if (status == bz2::kRanOut && more()) continue;
        if (status != bz2::kOk) return SLIMM_E_INVALID;
        bz2::link_block(ll.data(), info.n, counts.data(), link.data(), cf.data());
        const uint64_t text = bz2::text_length(link.data(), info.n, info.orig_ptr);
        if (text == bz2::kNoTextLength) return SLIMM_E_INVALID;
        decoded += text;
        bit = info.end_bit;
    }
    const uint64_t floor = std::min<uint64_t>(f.size, (bit + 7u) >> 3);
    slimm::even_ranges(floor, f.size, n, offsets_out, [](uint64_t t) { return t; });
    return SLIMM_OK;
}

// zstd is cut where a frame -- or a skippable frame -- starts, and nowhere else: frames are independent of each other (the
// window, the repeat offsets and the entropy tables start afresh at a frame header), and a frame cannot be entered in its
// middle.  The header's frames are decoded here (host/zstd.cpp) for the first legal cut; a cut is the first start at or
// behind its even share that zs::cut_candidate accepts (zstd_frame.h: the frame header parses, the block chain reaches the
// frame's end, a magic or the file's end stands behind it).  What the walk cannot see -- the blocks' contents -- the members
// and the stitch check.  The search for a cut gives up kZstdCutSearch bytes behind its target (SLIMM_FORCE zstd_cut_search=N):
// the cut is then the next one found, or the file's size, and the range in between is empty -- a file of one frame has all
// its cuts at its size, and member 0 reads it
constexpr uint64_t kZstdCutSearch = 64ull << 20;
int slimm_host_zstd_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    namespace zs = slimm::zs;
    if (!path || !n || !offsets_out || skip >= (1ull << 32)) return SLIMM_E_INVALID;
    slimm::PlanFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    auto read = [&](uint64_t off, uint8_t* dst, size_t k) { return off <= f.size && k <= f.size - off && f.read(off, dst, k); };
    // no cut in front of the end of the frame that holds decoded byte skip - 1: member 0 holds the whole header
    uint64_t first = 0;
    if (!slimm::zstd_header_end(read, f.size, skip, &first)) return SLIMM_E_INVALID;
    long v = 0;
    const uint64_t search = slimm::forced("zstd_cut_search", &v) && v > 0 ? static_cast<uint64_t>(v) : kZstdCutSearch;
    constexpr uint64_t kNone = slimm::kNoCut;
    std::vector<uint8_t> buf(1u << 20);
    // the first start at or behind t that is a cut, looked for in [t, t + search)
    auto cut_at = [&](uint64_t t) -> uint64_t {
        if (t >= f.size) return f.size;
        const uint64_t stop = std::min(f.size, t + search);
        for (uint64_t at = t; at < stop;) {
            const size_t k = static_cast<size_t>(std::min<uint64_t>(buf.size(), f.size - at));
            if (!f.read(at, buf.data(), k)) return kNone;
            for (size_t i = 0; i + 4u <= k && at + i < stop; ++i) {
                const uint8_t b = buf[i];
                if (b != 0x28u && (b & 0xf0u) != 0x50u) continue;
                const uint32_t magic = zs::le32(&buf[i]);
                uint64_t end = 0;
                if ((magic == zs::kMagic || (magic & 0xfffffff0u) == zs::kSkippable) && zs::cut_candidate(read, f.size, at + i, &end)) return at + i;
            }
            if (k < 4u) break;
            at += k - 3u;
        }
        return kNone;
    };
    slimm::even_ranges(first, f.size, n, offsets_out, cut_at);
    // (SLIMM_FORCE zstd_split_wrong_cut: the second cut -- the first of two members -- lands one byte late, where no frame
    // starts: the members, or the stitch, must refuse it)
    if (n > 1 && slimm::forced("zstd_split_wrong_cut")) {
        for (uint32_t i = std::min(2u, n - 1u); i >= 1u; --i) {
            const uint64_t was = offsets_out[i];
            if (was >= f.size || was == 0) continue;
            for (uint32_t j = i; j < n && offsets_out[j] == was; ++j) ++offsets_out[j];
            break;
        }
    }
    return SLIMM_OK;
}

uint64_t slimm_zstd_split_floor(void) {
    long v = 0;
    return slimm::forced("zstd_split_floor", &v) && v >= 0 ? static_cast<uint64_t>(v) : slimm::kZstdRoundBytes;
}

// xz is cut where its indexes say a block or a stream starts (host/xz.cpp: xz_plan_ranges): only the file's tail or tails
// are read -- footer, index, stream header, stream by stream from the file's end --, nothing is decoded and nothing guessed
int slimm_host_xz_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    if (!path || !n || !offsets_out || skip >= (1ull << 32)) return SLIMM_E_INVALID;
    slimm::PlanFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    auto read = [&](uint64_t off, uint8_t* dst, size_t k) { return off <= f.size && k <= f.size - off && f.read(off, dst, k); };
    return slimm::xz_plan_ranges(read, f.size, skip, n, offsets_out) ? SLIMM_OK : SLIMM_E_INVALID;
}

// gzip is cut at BITS: where a non-final dynamic block plausibly starts and a walk from there holds (gzip_plan.h).  The
// header's blocks are inflated here for the floor.  What the walk cannot see the members and the stitch check
int slimm_host_gzip_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* bit_offsets_out) {
    if (!path || !n || !bit_offsets_out || skip >= (1ull << 32)) return SLIMM_E_INVALID;
    slimm::PlanFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    auto read = [&](uint64_t off, uint8_t* dst, size_t k) { return off <= f.size && k <= f.size - off && f.read(off, dst, k); };
    slimm::GzipPlan plan;
    long v = 0;
    if (slimm::forced("gzip_cut_blocks", &v) && v > 0) plan.cut_blocks = static_cast<uint32_t>(v);
    if (slimm::forced("gzip_cut_search", &v) && v > 0) plan.cut_search = static_cast<uint64_t>(v);
    if (!slimm::gzip_plan_ranges(read, f.size, skip, n, bit_offsets_out, plan)) return SLIMM_E_INVALID;
    // (SLIMM_FORCE gzip_split_wrong_cut: the second cut -- the first of two members -- lands one bit late, where no block
    // starts: the members, or the stitch, must refuse it)
    if (n > 1 && slimm::forced("gzip_split_wrong_cut")) {
        for (uint32_t i = std::min(2u, n - 1u); i >= 1u; --i) {
            const uint64_t was = bit_offsets_out[i];
            if (was >= f.size * 8u || was == 0) continue;
            for (uint32_t j = i; j < n && bit_offsets_out[j] == was; ++j) ++bit_offsets_out[j];
            break;
        }
    }
    return SLIMM_OK;
}

// The least bytes per member at which the command cuts a gzip file for --split-input: zstd's, a stated default, NOT a
// measurement (SLIMM_FORCE gzip_split_floor=N)
uint64_t slimm_gzip_split_floor(void) {
    long v = 0;
    return slimm::forced("gzip_split_floor", &v) && v >= 0 ? static_cast<uint64_t>(v) : (32ull << 20);
}

int slimm_host_xz_check_at(const char* path, uint64_t offset, int* check_out) {
    if (!path || !check_out) return SLIMM_E_INVALID;
    slimm::PlanFile f;
    if (!f.open_regular(path)) return SLIMM_E_INVALID;
    auto read = [&](uint64_t off, uint8_t* dst, size_t k) { return off <= f.size && k <= f.size - off && f.read(off, dst, k); };
    return slimm::xz_check_at(read, f.size, offset, check_out) ? SLIMM_OK : SLIMM_E_INVALID;
}

// The least blocks per member at which the command cuts an xz file for --split-input: a range is decoded a lane per block,
// as a file is, so the floor is the same stated default as the command's kXzDeviceBlocks -- NOT a measurement: nothing is
// known yet of an LZMA lane's rate on the device (SLIMM_FORCE xz_split_blocks=N; a key of its own: xz_device_blocks decides
// whether the device reads the file at all)
constexpr uint64_t kXzSplitBlocks = 16;
uint64_t slimm_xz_split_floor(void) {
    long v = 0;
    return slimm::forced("xz_split_blocks", &v) && v >= 0 ? static_cast<uint64_t>(v) : kXzSplitBlocks;
}

}  // extern "C"

namespace slimm {

bool split_is_bzip2(const slimm_ctx* c) { return c->win.file.stream.codec == WindowPipeline::File::Codec::Bzip2; }

int split_bz2_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    auto rotl = [](uint32_t v, uint32_t k) {
        k &= 31u;
        return k ? (v << k) | (v >> (32u - k)) : v;
    };
    // the chain so far: where it ended, inside a stream of which level and combined CRC -- member 0's to begin with
    uint32_t left = 0;
    const WindowPipeline::File::Bzip2* L = &members[0]->win.file.bz2;
    bool in_stream = L->in_stream, at_file_end = L->chain.at_file_end;
    uint32_t level = L->level, combined = L->combined;
    uint64_t end_bit = L->chain.end_bit;
    for (uint32_t k = 1; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
        const WindowPipeline::File::Bzip2::Chain& K = Z.chain;
        if (!K.any) continue;   // (no block or marker starts in this range)
        *bad = k;
        if (!in_stream || end_bit != K.first_bit)
            return fail(c, SLIMM_E_SPLIT, "bzip2: the chain of member %u ends at bit %llu%s, this range's first block was found at bit %llu", left,
                        static_cast<unsigned long long>(end_bit), in_stream ? "" : " (behind the last stream)",
                        static_cast<unsigned long long>(K.first_bit));
        if (K.first_max_n > level * 100000u)
            return fail(c, SLIMM_E_INVALID, "bzip2-compressed input is not supported unless it decodes: block at byte %llu: %s",
                        static_cast<unsigned long long>(K.first_max_at), bz2::status_text(bz2::kTooLong));
        if (K.has_eos) {
            if ((rotl(combined, K.first_blocks) ^ K.first_combined) != K.eos_crc)
                return fail(c, SLIMM_E_INVALID, "bzip2-compressed input is not supported unless it decodes: end-of-stream marker at byte %llu: combined CRC mismatch",
                            static_cast<unsigned long long>(K.eos_at));
            level = Z.level;
            combined = Z.combined;
        } else {   // (no marker in this range: the stream goes on into the next)
            combined = rotl(combined, K.first_blocks) ^ Z.combined;
        }
        in_stream = Z.in_stream;
        at_file_end = K.at_file_end;
        end_bit = K.end_bit;
        left = k;
    }
    // the last chain ended the streams at the file's end (the file's last member checks that as one context does; a member
    // in front of it has seen every byte behind its last marker)
    *bad = left;
    if (left + 1 < n && !(at_file_end && !in_stream))
        return fail(members[left], SLIMM_E_SPLIT, "bzip2: the chain of member %u ends at bit %llu, and no range behind it holds a block", left,
                    static_cast<unsigned long long>(end_bit));
    return SLIMM_OK;
}

bool split_is_zstd(const slimm_ctx* c) { return c->win.file.stream.codec == WindowPipeline::File::Codec::Zstd; }

int split_zstd_ends(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    for (uint32_t k = 0; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::Announced& A = c->win.announced;
        const WindowPipeline::File::Stream& T = c->win.file.stream;
        const uint64_t at = T.base + (T.bit >> 3);   // (the file's byte its decoder stands at)
        *bad = k;
        if (!split_is_zstd(c) || !A.has_range)
            return fail(c, SLIMM_E_INVALID, "a range of a zstd file: slimm_set_input_range tells where it lies");
        if (c->win.file.zst.walk.stage != zs::Walker::Between || at != A.range_end || T.pend.size() != (T.bit >> 3))
            return fail(c, SLIMM_E_SPLIT, "zstd: the frames of member %u end at byte %llu, its range at byte %llu: the range does not end at a frame boundary", k,
                        static_cast<unsigned long long>(at), static_cast<unsigned long long>(A.range_end));
    }
    return SLIMM_OK;
}

bool split_is_xz(const slimm_ctx* c) { return c->win.file.stream.codec == WindowPipeline::File::Codec::Xz; }

int split_xz_streams(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    using XF = WindowPipeline::File::Xz;
    // the stream that lies over the cut in front of member k: its check kind and its blocks in the ranges on the left
    bool open = false;
    uint32_t check = 0;
    std::vector<std::pair<uint64_t, uint64_t>> blocks;
    for (uint32_t k = 0; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::Announced& A = c->win.announced;
        const WindowPipeline::File::Stream& T = c->win.file.stream;
        const XF& Z = c->win.file.xz;
        const uint64_t at = T.base + (T.bit >> 3);   // (the file's byte its walker stands at)
        *bad = k;
        if (!split_is_xz(c) || !A.has_range) return fail(c, SLIMM_E_INVALID, "a range of an xz file: slimm_set_input_range tells where it lies");
        if (at != A.range_end || T.pend.size() != (T.bit >> 3) || !Z.ready.empty())
            return fail(c, SLIMM_E_SPLIT, "xz: the blocks of member %u end at byte %llu, its range at byte %llu: the range does not end at a block boundary", k,
                        static_cast<unsigned long long>(at), static_cast<unsigned long long>(A.range_end));
        if (Z.from_left != open)
            return fail(c, SLIMM_E_SPLIT, open ? "xz: member %u starts at a stream header, and the stream on its left has not ended"
                                               : "xz: member %u was told a check kind, and no stream lies over the cut in front of it", k);
        if (Z.from_left && Z.walk.check != check && Z.walk.open_left)
            return fail(c, SLIMM_E_SPLIT, "xz: member %u was told check kind %u, the stream's header states %u", k, static_cast<unsigned>(Z.walk.check),
                        static_cast<unsigned>(check));
        if (Z.from_left && !Z.walk.open_left) {   // (its footer's kind was the told one: xz_round)
            if (static_cast<uint32_t>(A.xz_check) != check)
                return fail(c, SLIMM_E_SPLIT, "xz: member %u was told check kind %d, the stream's header states %u", k, A.xz_check, static_cast<unsigned>(check));
            if (blocks != Z.left_kept)
                return fail(c, SLIMM_E_INVALID, "xz-compressed input is not supported unless it decodes: index at byte %llu: %s",
                            static_cast<unsigned long long>(Z.left_index_at), xz::status_text(xz::kIndexMismatch));
            open = false;
            blocks.clear();
        }
        if (Z.walk.stage == xz::Walker::Blocks) {   // (the range ends among a stream's blocks)
            if (!open) check = Z.walk.check;
            open = true;
            blocks.insert(blocks.end(), Z.walk.records.begin(), Z.walk.records.end());
        }
    }
    *bad = n - 1u;
    if (open) return fail(members[n - 1u], SLIMM_E_SPLIT, "xz: the last range ends among a stream's blocks");
    return SLIMM_OK;
}

bool split_is_gzip(const slimm_ctx* c) { return c->win.file.stream.codec == WindowPipeline::File::Codec::Gzip; }

namespace {
// where a member's chain stands, as a bit of the file
uint64_t gz_chain_end(const slimm_ctx* c) {
    const WindowPipeline::Announced& A = c->win.announced;
    const WindowPipeline::File::Stream& T = c->win.file.stream;
    return A.gz_begin_bit == A.gz_end_bit ? A.gz_begin_bit : T.base * 8u + T.bit;
}
int gz_chain_ended(slimm_ctx* c, uint32_t k, uint64_t want) {
    if (c->win.file.gz.range_done && gz_chain_end(c) == want) return SLIMM_OK;
    return fail(c, SLIMM_E_SPLIT, "gzip: the chain of member %u ended at bit %llu, its range at bit %llu", k,
                static_cast<unsigned long long>(gz_chain_end(c)), static_cast<unsigned long long>(want));
}
}  // namespace

int split_gz_windows(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    using GF = WindowPipeline::File::Gzip;
    std::vector<bool> ran(n, false);
    for (uint32_t k = 0; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::File& F = c->win.file;
        *bad = k;
        // (the last member, which may do without the window pass, may announce its range behind this call)
        if (!c->win.announced.gz_range && (k + 1u < n || F.active)) return fail(c, SLIMM_E_INVALID, "a range of a gzip file: slimm_set_gzip_range tells where it lies");
        ran[k] = F.active && F.closed && split_is_gzip(c) && F.gz.window_pass;
        if (F.active && !ran[k]) return fail(c, SLIMM_E_INVALID, "slimm_group_gzip_windows: behind the members' window pass (slimm_set_gzip_window_pass), pushed to its end");
        if (!ran[k] && k + 1u < n) return fail(c, SLIMM_E_INVALID, "slimm_group_gzip_windows: only the last member may do without the window pass");
    }
    bool open = false;   // a gzip member lies over the cut behind member k
    for (uint32_t k = 0; k + 1u < n; ++k) {
        slimm_ctx *c = members[k], *r = members[k + 1u];
        WindowPipeline& W = c->win;
        WindowPipeline::Gzip& S = W.gz;
        const WindowPipeline::Announced &A = W.announced, &AR = r->win.announced;
        const GF& Z = W.file.gz;
        const bool empty = A.gz_begin_bit == A.gz_end_bit;
        *bad = k;
        const bool told = AR.gz_range;
        if (told && A.gz_end_bit != AR.gz_begin_bit)
            return fail(c, SLIMM_E_INVALID, "slimm_group_gzip_windows: member %u's range ends at bit %llu, member %u's begins at bit %llu", k,
                        static_cast<unsigned long long>(A.gz_end_bit), k + 1u, static_cast<unsigned long long>(AR.gz_begin_bit));
        SLIMM_TRY(gz_chain_ended(c, k, A.gz_end_bit));
        uint32_t front_len = 0;
        if (!empty) {
            open = Z.stage == GF::Deflate;
            front_len = static_cast<uint32_t>(std::min<uint64_t>(gz::kWindow, (Z.partial ? W.gz_pass.front_len : 0u) + Z.len));
            if (!open) front_len = 0;
        } else {
            front_len = W.gz_pass.front_len;
        }
        if (!open && told && AR.gz_begin_bit != AR.gz_end_bit)
            return fail(c, SLIMM_E_SPLIT, "gzip: the chain of member %u ended between two gzip members at bit %llu, where member %u's range begins among blocks", k,
                        static_cast<unsigned long long>(gz_chain_end(c)), k + 1u);
        // the bytes in front of member k + 1: k's final window, its markers filled from the bytes in front of k
        (void)hipSetDevice(c->device);
        HIP_TRY(c, S.front.ensure(gz::kWindow));
        HIP_TRY(c, S.applied.ensure(gz::kWindow));
        if (!W.gz_pass.has_front) HIP_TRY(c, hipMemsetAsync(S.front.p, 0, gz::kWindow, c->stream));   // (member 0: nothing in front)
        if (Z.carried) {
            launch_gz_window_apply(c->stream, S.win16.p, S.front.p, S.applied.p);
            HIP_TRY(c, hipGetLastError());
        } else {   // (no chunk in this range: what lies in front of it lies in front of the next)
            HIP_TRY(c, hipMemcpyAsync(S.applied.p, S.front.p, gz::kWindow, hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        (void)hipSetDevice(r->device);
        HIP_TRY(r, r->win.gz.front.ensure(gz::kWindow));
        if (r->device == c->device)
            HIP_TRY(r, hipMemcpyAsync(r->win.gz.front.p, S.applied.p, gz::kWindow, hipMemcpyDeviceToDevice, r->stream));
        else
            HIP_TRY(r, hipMemcpyPeerAsync(r->win.gz.front.p, r->device, S.applied.p, c->device, gz::kWindow, r->stream));
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        r->win.gz_pass.has_front = true;
        r->win.gz_pass.front_len = front_len;
        W.gz_pass.done = true;
        W.gz_pass.end_bit = gz_chain_end(c);
        W.gz_pass.text = Z.text;
    }
    for (uint32_t k = 0; k < n; ++k) {   // the text pass starts from a fresh file, told what the window pass was told
        if (!ran[k]) continue;
        slimm_ctx* c = members[k];
        *bad = k;
        if (k + 1u == n) {
            c->win.gz_pass.done = true;
            c->win.gz_pass.end_bit = gz_chain_end(c);
            c->win.gz_pass.text = c->win.file.gz.text;
        }
        WindowPipeline::Announced a = c->win.announced;
        const WindowPipeline::GzipPass p = c->win.gz_pass;
        a.gz_window_pass = false;
        (void)hipSetDevice(c->device);
        SLIMM_TRY(c->win.end_file(c));
        c->win.announced = a;
        c->win.gz_pass = p;
    }
    return SLIMM_OK;
}

int split_gz_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    using GF = WindowPipeline::File::Gzip;
    bool open = false;          // a gzip member lies over the cut in front of member k:
    uint32_t s = 0;             // its CRC register and its length up to the cut
    uint64_t len = 0;
    for (uint32_t k = 0; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::Announced& A = c->win.announced;
        const WindowPipeline::GzipPass& P = c->win.gz_pass;
        const GF& Z = c->win.file.gz;
        const bool empty = A.gz_begin_bit == A.gz_end_bit;
        *bad = k;
        if (!split_is_gzip(c) || !A.gz_range) return fail(c, SLIMM_E_INVALID, "a range of a gzip file: slimm_set_gzip_range tells where it lies");
        if (Z.window_pass) return fail(c, SLIMM_E_INVALID, "a range of a gzip file: slimm_group_gzip_windows and the text pass come before the stitch");
        if (k && A.gz_begin_bit != members[k - 1u]->win.announced.gz_end_bit)
            return fail(c, SLIMM_E_INVALID, "a range of a gzip file: member %u's range begins at bit %llu, member %u's ends at bit %llu", k,
                        static_cast<unsigned long long>(A.gz_begin_bit), k - 1u, static_cast<unsigned long long>(members[k - 1u]->win.announced.gz_end_bit));
        if (k + 1u < n) SLIMM_TRY(gz_chain_ended(c, k, A.gz_end_bit));
        if (P.done && (P.end_bit != gz_chain_end(c) || P.text != Z.text))
            return fail(c, SLIMM_E_SPLIT, "gzip: the window pass of member %u ended at bit %llu behind %llu bytes of text, its text pass at bit %llu behind %llu", k,
                        static_cast<unsigned long long>(P.end_bit), static_cast<unsigned long long>(P.text),
                        static_cast<unsigned long long>(gz_chain_end(c)), static_cast<unsigned long long>(Z.text));
        if (empty && k) continue;   // (it hands on what it was handed)
        if (A.starts_mid && k) {
            if (!open)
                return fail(c, SLIMM_E_SPLIT, "gzip: member %u's range begins among blocks, and no gzip member lies over the cut in front of it", k);
            if (Z.left.has) {   // the member's trailer, read here: its parts on the left and this range's against it
                s = gz::crc_mul(s, gz::crc_x_pow8(Z.left.partial_len)) ^ Z.left.partial_crc;
                len += Z.left.partial_len;
                if (Z.left.crc32 != ~s)
                    return fail(c, SLIMM_E_INVALID, "corrupt gzip stream (%s): the trailer at byte %llu of a member that lies over a cut", gz::status_text(gz::kBadCrc),
                                static_cast<unsigned long long>(Z.left.at));
                if (Z.left.isize != static_cast<uint32_t>(len))
                    return fail(c, SLIMM_E_INVALID, "corrupt gzip stream (%s): the trailer at byte %llu of a member that lies over a cut", gz::status_text(gz::kBadLength),
                                static_cast<unsigned long long>(Z.left.at));
            } else {   // (no trailer in this range: both go on)
                s = gz::crc_mul(s, gz::crc_x_pow8(Z.len)) ^ Z.crc;
                len += Z.len;
                continue;
            }
        }
        open = Z.stage == GF::Deflate;
        s = Z.crc;
        len = Z.len;
    }
    return SLIMM_OK;
}

int split_range(slimm_ctx* c, SplitRange* out) {
    if (!c || !out) return SLIMM_E_INVALID;
    if (c->device < 0 || !c->win.file.active || !c->win.file.closed)
        return fail(c, SLIMM_E_INVALID, "a range of a split file: a range of BAM, SAM, BGZF SAM, bzip2 SAM, zstd SAM or xz SAM pushed to its end");
    if (split_is_bzip2(c) && !c->win.announced.has_range)
        return fail(c, SLIMM_E_INVALID, "a range of a bzip2 file: slimm_set_input_range tells where it lies");
    if (split_is_xz(c) && !c->win.announced.has_range)
        return fail(c, SLIMM_E_INVALID, "a range of an xz file: slimm_set_input_range tells where it lies");
    out->found_start = c->win.file.found_start || !c->win.announced.starts_mid;
    out->head_len = c->win.announced.starts_mid ? c->win.file.head_len : 0u;
    out->n_records = c->n_pushed;
    return SLIMM_OK;
}

int split_append_head(slimm_ctx* left, slimm_ctx* right, bool final, uint64_t* n_records) {
    (void)hipSetDevice(right->device);
    HIP_TRY(right, hipStreamSynchronize(right->stream));   // (the head was copied aside on the right member's stream)
    const uint64_t n = right->win.announced.starts_mid ? right->win.file.head_len : 0u;
    uint64_t got = 0;
    // SAM: the file's last range inflated to nothing (it is empty, or holds the EOF block only), so no member has ended a
    // last line that lacks its newline: the member that holds the line does
    const bool end_line = left->win.file.sam && !right->win.announced.ends_mid && !right->win.file.windows && left->win.file.carry_bytes;
    SLIMM_TRY(append_window(left, right->win.head_bytes.p, right->device, n, final, got, end_line));
    HIP_TRY(left, hipStreamSynchronize(left->stream));
    if (n_records) *n_records = got;
    return SLIMM_OK;
}

int split_join(slimm_ctx* left, slimm_ctx* right) {
    WindowPipeline& R = right->win;
    if (!R.file.has_first || !right->n_pushed || !left->win.carry.p) return SLIMM_OK;   // (nothing on one side: no run to join)
    (void)hipSetDevice(left->device);
    HIP_TRY(left, hipStreamSynchronize(left->stream));
    (void)hipSetDevice(right->device);
    HIP_TRY(right, R.join.ensure(1));
    if (left->device == right->device)
        HIP_TRY(right, hipMemcpyAsync(R.join.p, left->win.carry.p, sizeof(BamCarry), hipMemcpyDeviceToDevice, right->stream));
    else
        HIP_TRY(right, hipMemcpyPeerAsync(R.join.p, right->device, left->win.carry.p, left->device, sizeof(BamCarry), right->stream));
    launch_split_join(right->stream, R.join.p, R.first.p, R.carry.p, reinterpret_cast<uint32_t*>(right->in_ref.p));
    HIP_TRY(right, hipGetLastError());
    HIP_TRY(right, hipStreamSynchronize(right->stream));
    return SLIMM_OK;
}

int split_first_start(slimm_ctx* c, uint64_t* index) {
    const uint64_t n = c->n_pushed;
    *index = n;
    if (!n) return SLIMM_OK;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, c->win.guess.ensure(1));
    unsigned long long v = n;
    HIP_TRY(c, hipMemcpyAsync(c->win.guess.p, &v, sizeof(v), hipMemcpyHostToDevice, c->stream));
    launch_split_first_start(c->stream, reinterpret_cast<const uint32_t*>(c->in_ref.p), n, c->win.guess.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&v, c->win.guess.p, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *index = v;
    return SLIMM_OK;
}

int split_take(slimm_ctx* dst, slimm_ctx* src, uint64_t n) {
    if (!n) return SLIMM_OK;
    if (n > src->n_pushed) return fail(dst, SLIMM_E_INVALID, "split_take: more records than the member holds");
    if (dst->n_pushed + n >= record_cap()) return fail(dst, SLIMM_E_INVALID, "a context handles fewer than 2^31 records; shard the stream");
    (void)hipSetDevice(src->device);
    HIP_TRY(src, hipStreamSynchronize(src->stream));
    (void)hipSetDevice(dst->device);
    SLIMM_TRY(slimm_reserve(dst, dst->n_pushed + n));
    const uint64_t at = dst->n_pushed;
    if (dst->device == src->device) {
        HIP_TRY(dst, hipMemcpyAsync(dst->in_ref.p + at, src->in_ref.p, n * 4, hipMemcpyDeviceToDevice, dst->stream));
        HIP_TRY(dst, hipMemcpyAsync(dst->in_pos.p + at, src->in_pos.p, n * 4, hipMemcpyDeviceToDevice, dst->stream));
    } else {
        HIP_TRY(dst, hipMemcpyPeerAsync(dst->in_ref.p + at, dst->device, src->in_ref.p, src->device, n * 4, dst->stream));
        HIP_TRY(dst, hipMemcpyPeerAsync(dst->in_pos.p + at, dst->device, src->in_pos.p, src->device, n * 4, dst->stream));
    }
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    dst->n_pushed += n;
    return SLIMM_OK;
}

int split_keep(slimm_ctx* c, uint64_t from) {
    if (from > c->n_pushed) return fail(c, SLIMM_E_INVALID, "split_keep: past the member's records");
    c->marked = true;
    view_records(c, from);
    c->win.file.q18_by_group = true;
    return SLIMM_OK;
}

void group_filter_peers(slimm_ctx* member0, slimm_ctx* const* others, uint32_t n) { member0->filter_peers.assign(others, others + n); }

}  // namespace slimm
