// One file split by byte range over a group's members (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE"): the host's plans
// of the ranges (slimm_host_*_ranges, on split_plan.h) and the codec-neutral steps of slimm_group_stitch_ranges (split.h;
// group.hip runs them cut by cut).  A streamed codec's own check in the stitch is its row of kCodecs (windows.h) and lies with
// its decoder.  Where each form is cut, and how a range that starts inside the file finds its start:
//   BAM        at BGZF blocks; the first record is guessed (bam_decode.hip: k_bam_first_guess), the left member confirms it
//   SAM        anywhere; the first line starts behind the first newline (sam_decode.hip: k_sam_first_newline)
//   BGZF SAM   at BGZF blocks; text from there on, as SAM
//   bzip2 SAM  anywhere; the range starts at its first block, the chains of blocks are held together (bzip2_decode.hip)
//   zstd SAM   where frames start; every member's frames must end at its range's end (zstd_decode.hip)
//   xz SAM     at a stream header or a block, by the indexes; a stream over cuts is held against its index (xz_decode.hip)
//   gzip SAM   at the BITS where dynamic blocks start; two passes, the windows handed on in between (gzip_decode.hip)
// The left member's incomplete last record (line) followed by the right member's head must be whole records (lines) that end
// exactly where the right member's first begins.  The reference reads one file with one reader (src/misc.hpp:498-522).
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

// a planner's frame: its arguments are there, the header fits the first push's 32-bit `skip` (bgzf, bzip2: not asked), and
// the file is a regular one, now open
bool plan_opens(slimm::PlanFile& f, const char* path, uint32_t n, const uint64_t* offsets_out, uint64_t skip = 0) {
    return path && n && offsets_out && skip < (1ull << 32) && f.open_regular(path);
}

}  // namespace

extern "C" {

uint64_t slimm_record_cap(void) { return slimm::record_cap(); }

int slimm_host_bgzf_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    BgzfFile f;
    if (!plan_opens(f, path, n, offsets_out)) return SLIMM_E_INVALID;
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
    slimm::PlanFile f;
    if (!plan_opens(f, path, n, offsets_out)) return SLIMM_E_INVALID;
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
    slimm::PlanFile f;
    if (!plan_opens(f, path, n, offsets_out, skip)) return SLIMM_E_INVALID;
    const auto read = f.reader();
    // no cut in front of the end of the frame that holds decoded byte skip - 1: member 0 holds the whole header
    uint64_t first = 0;
    if (!slimm::zstd_header_end(read, f.size, skip, &first)) return SLIMM_E_INVALID;
    const uint64_t search = slimm::forced_or("zstd_cut_search", kZstdCutSearch, 1);
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
    if (slimm::forced("zstd_split_wrong_cut")) slimm::force_wrong_cut(offsets_out, n, f.size);   // (one byte late: no frame starts there)
    return SLIMM_OK;
}

uint64_t slimm_zstd_split_floor(void) { return slimm::forced_or("zstd_split_floor", slimm::kZstdRoundBytes); }

// xz is cut where its indexes say a block or a stream starts (host/xz.cpp: xz_plan_ranges): only the file's tail or tails
// are read -- footer, index, stream header, stream by stream from the file's end --, nothing is decoded and nothing guessed
int slimm_host_xz_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out) {
    slimm::PlanFile f;
    if (!plan_opens(f, path, n, offsets_out, skip)) return SLIMM_E_INVALID;
    return slimm::xz_plan_ranges(f.reader(), f.size, skip, n, offsets_out) ? SLIMM_OK : SLIMM_E_INVALID;
}

// gzip is cut at BITS: where a non-final dynamic block plausibly starts and a walk from there holds (gzip_plan.h).  The
// header's blocks are inflated here for the floor.  What the walk cannot see the members and the stitch check
int slimm_host_gzip_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* bit_offsets_out) {
    slimm::PlanFile f;
    if (!plan_opens(f, path, n, bit_offsets_out, skip)) return SLIMM_E_INVALID;
    slimm::GzipPlan plan;
    plan.cut_blocks = static_cast<uint32_t>(slimm::forced_or("gzip_cut_blocks", plan.cut_blocks, 1));
    plan.cut_search = slimm::forced_or("gzip_cut_search", plan.cut_search, 1);
    if (!slimm::gzip_plan_ranges(f.reader(), f.size, skip, n, bit_offsets_out, plan)) return SLIMM_E_INVALID;
    if (slimm::forced("gzip_split_wrong_cut")) slimm::force_wrong_cut(bit_offsets_out, n, f.size * 8u);   // (one bit late: no block starts there)
    return SLIMM_OK;
}

// The least bytes per member at which the command cuts a gzip file for --split-input: zstd's, a stated default, NOT a
// measurement (SLIMM_FORCE gzip_split_floor=N)
uint64_t slimm_gzip_split_floor(void) { return slimm::forced_or("gzip_split_floor", 32ull << 20); }

int slimm_host_xz_check_at(const char* path, uint64_t offset, int* check_out) {
    slimm::PlanFile f;
    if (!path || !check_out || !f.open_regular(path)) return SLIMM_E_INVALID;
    return slimm::xz_check_at(f.reader(), f.size, offset, check_out) ? SLIMM_OK : SLIMM_E_INVALID;
}

// The least blocks per member at which the command cuts an xz file for --split-input: a range is decoded a lane per block,
// as a file is, so the floor is the same stated default as the command's kXzDeviceBlocks -- NOT a measurement: nothing is
// known yet of an LZMA lane's rate on the device (SLIMM_FORCE xz_split_blocks=N; a key of its own: xz_device_blocks decides
// whether the device reads the file at all)
constexpr uint64_t kXzSplitBlocks = 16;
uint64_t slimm_xz_split_floor(void) { return slimm::forced_or("xz_split_blocks", kXzSplitBlocks); }

}  // extern "C"

namespace slimm {

int split_range(slimm_ctx* c, SplitRange* out) {
    if (!c || !out) return SLIMM_E_INVALID;
    if (c->device < 0 || !c->win.file.active || !c->win.file.closed)
        return fail(c, SLIMM_E_INVALID, "a range of a split file: a range of BAM, SAM, BGZF SAM, bzip2 SAM, zstd SAM or xz SAM pushed to its end");
    const StreamCodec& K = codec_of(c->win.file.stream.codec);
    if (K.range_announced && !c->win.announced.has_range)
        return fail(c, SLIMM_E_INVALID, "a range of %s %s file: slimm_set_input_range tells where it lies", K.article ? K.article : "a", K.name);
    out->found_start = c->win.file.found_start || !c->win.announced.starts_mid;
    out->head_len = c->win.announced.starts_mid ? c->win.file.head_len : 0u;
    out->n_records = c->n_pushed;
    return SLIMM_OK;
}

int split_codec_stitch(slimm_ctx* const* members, uint32_t n, uint32_t* bad, const char** split_words, const char** noun) {
    const StreamCodec& K = codec_of(members[0]->win.file.stream.codec);
    *split_words = K.stitch_split;
    *noun = K.stitch_noun;
    return K.stitch ? K.stitch(members, n, bad) : SLIMM_OK;
}

int split_codec_windows(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    const StreamCodec& K = codec_of(members[0]->win.file.stream.codec);
    return (K.window_stitch ? K.window_stitch : split_gz_windows)(members, n, bad);
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
