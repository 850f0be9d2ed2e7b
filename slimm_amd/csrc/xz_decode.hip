// xz-compressed SAM decoded on the device (include/slimm_hip.h: slimm_push_xz_sam_bytes; the format: xz_stream.h).
// A stream is a sequence of blocks, each with an empty dictionary and fresh LZMA state in front of it, and every LZMA2 chunk
// states its compressed and its uncompressed size: the host walks a block from chunk header to chunk header without decoding
// a bit, and knows every block's extent and the exact place of its text before a kernel runs.  The bytes at hand go through
// stages, a ROUND:
//   (host)        what lies between blocks read -- stream header, block header, index (against the blocks walked since the
//                 stream header), footer, padding --; of every whole block at hand the chunk chain walked to its end marker,
//                 its padding and check field found; the text offsets are a prefix sum of the chunks' stated sizes
//   k_xz_decode   a workgroup of one wave per block, the probabilities in LDS: all lanes read the chunk headers, set the
//                 probabilities at a state reset and copy uncompressed chunks; the FIRST lane decodes the LZMA chunks, straight
//                 to the block's place in the round's text -- which is its dictionary: a match copies from the block's own
//                 earlier output
//   k_xz_check    a thread per gz::kPiece bytes of text: the block's CRC32 or CRC64 register over the piece, from 0;
//   k_xz_fold     a thread per block sums its pieces (xz_stream.h: crc64_mul; deflate_stream.h: crc_mul)
//   (host)        the registers against the blocks' check fields.  SHA-256 is NOT verified: such blocks are counted
// A byte range of a split file (include/slimm_hip.h, "xz SAM by byte range") changes the host's walk alone: where it starts --
// at a stream header, or among a stream's blocks with the check kind it was told --, where it must stop, and what it keeps of
// an index whose first records are blocks of the ranges on its left (split.hip: split_xz_streams holds them against those).
// No workgroup waits for another.  One round is one window; the window then goes to the SAM finder and decoder as any text
// window does (windows.hip).  NOT MEASURED on an MI355X: nothing is known of an LZMA lane's rate there.
#include "context.h"

namespace slimm {
namespace {

constexpr uint64_t kXzTail = 16;                    // zeroed bytes behind the compressed bytes on the device
constexpr uint64_t kXzRoundText = 512ull << 20;     // a round's text at most (SLIMM_FORCE xz_round_text=N), or one block alone
constexpr uint64_t kXzBlockTextMax = 1ull << 30;    // one block of more text than that is refused
using XF = WindowPipeline::File::Xz;
using Stage = XF::Stage;

// (a decoder is ONE lane of a wave of its own, as k_gz_decode's and k_bz2_decode's: lanes of one wave that decode different
// blocks would take each other's branches in turn, and a file has far fewer blocks than the device has waves.  The 28 268
// bytes of probabilities let five such workgroups share a CU's LDS)
__global__ __launch_bounds__(64) void k_xz_decode(const uint8_t* __restrict__ comp, uint64_t n_bytes, xz::Block* __restrict__ blocks, uint32_t n,
                                                   uint8_t* __restrict__ text) {
    __shared__ uint16_t probs[xz::kProbsMax];
    __shared__ uint32_t status;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    xz::Block& b = blocks[i];
    const uint64_t b_end = b.end, text_len = b.text_len;
    uint8_t* const mine = text + b.text_at;
    xz::Lzma s{};
    xz::Rules rules;
    xz::Tally tally{0, 0};
    uint32_t counts[5] = {0, 0, 0, 0, 0};   // LZMA chunks, uncompressed chunks, state resets, properties changes, ... not the default
    uint64_t at = b.at, out = 0, since = 0;
    uint32_t st = b_end <= n_bytes && at < b_end ? xz::kOk : xz::kOverrun;
    if (lane == 0) status = xz::kOk;
    __syncthreads();
    while (st == xz::kOk) {
        xz::Chunk ch;
        st = xz::chunk_header(comp + at, b_end - at, rules, ch);   // (the same for every lane)
        if (st != xz::kOk) break;
        if (ch.control == 0) {
            if (out != text_len || at + 1u != b_end) st = xz::kOverrun;
            break;
        }
        if (ch.usize > text_len - out || static_cast<uint64_t>(ch.header) + ch.csize > b_end - at) {
            st = xz::kOverrun;
            break;
        }
        uint8_t* dst = mine + out;
        const uint8_t* src = comp + at + ch.header;
        if (ch.dict_reset) since = 0;
        if (!ch.lzma) {
            for (uint32_t k = lane; k < ch.usize; k += 64u) dst[k] = src[k];
            ++counts[1];
        } else {
            if (ch.new_props) {
                s.lc = ch.lc, s.lp = ch.lp, s.pb = ch.pb;
                ++counts[3];
                if (ch.props != 0x5du) ++counts[4];
            }
            if (ch.state_reset) {
                s.reset_state();
                const uint32_t np = xz::n_probs(s.lc, s.lp);
                for (uint32_t k = lane; k < np; k += 64u) probs[k] = xz::kProbInit;
                ++counts[2];
            }
            ++counts[0];
            __syncthreads();   // (the probabilities, and the bytes the other lanes copied in front of this chunk)
            if (lane == 0) {
                xz::Rc rc;
                uint32_t r = rc.init(src, 0, ch.csize);
                if (r == xz::kOk) r = xz::lzma_chunk(rc, s, probs, dst, ch.usize, since, b.dict_size, tally);
                status = r;
            }
        }
        __syncthreads();
        st = status;
        since += ch.usize;
        out += ch.usize;
        at += static_cast<uint64_t>(ch.header) + ch.csize;
    }
    if (lane == 0) {
        b.status = st;
        b.lzma_chunks = counts[0], b.raw_chunks = counts[1], b.state_resets = counts[2], b.prop_changes = counts[3], b.odd_props = counts[4];
        b.match_bytes = tally.match_bytes;
        b.max_dist = tally.max_dist;
    }
}

__global__ __launch_bounds__(256) void k_xz_check(const xz::Block* __restrict__ blocks, uint32_t n, uint32_t n_pieces, const uint8_t* __restrict__ text,
                                                   xz::Piece* __restrict__ piece) {
    __shared__ uint32_t t32[256];
    __shared__ uint64_t t64[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) t32[i] = gz::crc_table_entry(i), t64[i] = xz::crc64_table_entry(i);
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    uint32_t lo = 0, hi = n;   // the block of piece p: the last one whose piece0 <= p (a block of no text has no piece)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (blocks[mid].piece0 <= p) lo = mid; else hi = mid;
    }
    const xz::Block& b = blocks[lo];
    const uint64_t from = static_cast<uint64_t>(p - b.piece0) * gz::kPiece;
    const uint64_t to = from + gz::kPiece < b.text_len ? from + gz::kPiece : b.text_len;
    const uint8_t* t = text + b.text_at;
    uint64_t reg = 0;
    if (b.check == xz::kCheckCrc32) {
        uint32_t c = 0;
        for (uint64_t j = from; j < to; ++j) c = t32[(c ^ t[j]) & 0xffu] ^ (c >> 8);
        reg = c;
    } else if (b.check == xz::kCheckCrc64) {
        for (uint64_t j = from; j < to; ++j) reg = t64[(reg ^ t[j]) & 0xffu] ^ (reg >> 8);
    }
    piece[p] = xz::Piece{reg, 0};
}

__global__ __launch_bounds__(64) void k_xz_fold(xz::Block* __restrict__ blocks, uint32_t n, const xz::Piece* __restrict__ piece, uint32_t full32,
                                                 uint64_t full64) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xz::Block& b = blocks[i];
    const uint32_t np = static_cast<uint32_t>((b.text_len + gz::kPiece - 1u) / gz::kPiece);
    uint64_t reg = 0;
    if (b.check == xz::kCheckCrc32) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < np; ++j)
            c = gz::crc_mul(c, j + 1u == np ? static_cast<uint32_t>(b.last_mul) : full32) ^ static_cast<uint32_t>(piece[b.piece0 + j].reg);
        reg = c;
    } else if (b.check == xz::kCheckCrc64) {
        for (uint32_t j = 0; j < np; ++j) reg = xz::crc64_mul(reg, j + 1u == np ? b.last_mul : full64) ^ piece[b.piece0 + j].reg;
    }
    b.crc = reg;
}

void push_trace_xz(const char* fmt, ...) {   // "[push xz] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("xz", fmt, ap);
    va_end(ap);
}

// the host reader's words (host/alignment_file.cpp: codec_read)
int xz_fail(slimm_ctx* c, const std::string& where, uint32_t status, const std::string& more = "") {
    return fail(c, SLIMM_E_INVALID, "xz-compressed input is not supported unless it decodes: %s: %s%s", where.c_str(), xz::status_text(status), more.c_str());
}

// inside xz_round's loop: the error now, or -- behind blocks that are ready -- once they are decoded
#define XZ_FAIL(call)                \
    {                                \
        if (!Z.ready.empty()) break; \
        return call;                 \
    }

bool all_zero(const uint8_t* p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

}  // namespace

bool xz_next_window(const slimm_ctx* c, uint64_t, uint64_t* n) {   // (a round's text is one window: kXzRoundText)
    const XF& Z = c->win.file.xz;
    *n = Z.text - std::min(Z.text, c->win.file.stream.skip_left);
    return !Z.ready.empty();
}

int xz_round(slimm_ctx* c, bool last) {
    WindowPipeline& W = c->win;
    XF& Z = W.file.xz;
    WindowPipeline::File::Stream& T = W.file.stream;
    uint64_t* stats = W.xz_stats;
    Z.ready.clear(), Z.ready_at.clear();
    Z.text = 0;
    if (T.waiting && !last) return SLIMM_OK;
    T.waiting = false;   // (at the file's end what waited for bytes is looked at again: it ends the streams, or is truncated)
    // (xz reads at bytes: `pos` is the stream's bit, put back however the round ends)
    uint64_t pos = T.bit >> 3;
    struct PutBack {
        uint64_t &bit, &pos;
        ~PutBack() { bit = pos * 8u; }
    } put_back{T.bit, pos};
    long cap_text = 0;
    if (!forced("xz_round_text", &cap_text) || cap_text <= 0) cap_text = static_cast<long>(kXzRoundText);
    auto at = [&](uint64_t byte) { return std::to_string(T.base + byte); };
    // a byte range of a split file (check_push: its range is announced).  It starts at a stream header or -- told the check
    // kind of the stream around it, which sizes the field behind every block -- at a block's first byte, and ends at a
    // block's first byte or between streams, or the cut is refused: SLIMM_E_SPLIT, no verdict on the file
    const WindowPipeline::Announced& A = W.announced;
    const bool starts_mid = A.has_range && A.starts_mid, ends_mid = A.has_range && A.ends_mid;
    auto no_start = [&](uint64_t byte, const char* what) {
        return fail(c, SLIMM_E_SPLIT, "xz: the range starts at byte %s, where no %s starts", at(byte).c_str(), what);
    };
    auto no_end = [&](const std::string& where) {
        return fail(c, SLIMM_E_SPLIT, "xz: %s runs past byte %llu: the range does not end at a block boundary", where.c_str(),
                    static_cast<unsigned long long>(A.range_end));
    };
    if (!Z.started) {
        Z.started = true;
        if (starts_mid && A.xz_check >= 0) {   // (among the blocks of a stream whose header lies in a range on the left)
            Z.stage = Stage::Blocks;
            Z.check = static_cast<uint32_t>(A.xz_check);
            Z.from_left = true;
            Z.any_streams = 1;
        }
    }
    // what a step lacks: more bytes may come, or the file ends inside it
    // (errors come in file order: what is wrong behind blocks that are ready is looked at again by the next round, once
    // those blocks are decoded -- nothing is read past it: XZ_FAIL)
    auto wait_or = [&](const std::string& where) {
        if (last && Z.ready.empty()) return ends_mid ? no_end(where) : xz_fail(c, where, xz::kRanOut);
        if (!last) T.waiting = true;
        return static_cast<int>(SLIMM_OK);
    };
    const uint64_t n_bytes = T.pend.size();
    const uint8_t* p = T.pend.data();
    uint64_t text = 0;
    uint32_t pieces = 0;
    while (!T.waiting) {
        uint64_t avail = n_bytes - pos;
        if (Z.stage == Stage::Between) {
            while (Z.any_streams > 0 && avail >= 4u && all_zero(p + pos, 4)) pos += 4u, avail -= 4u;   // (stream padding)
            if (avail < xz::kHeaderBytes) {
                if (!last || (avail == 0 && (Z.any_streams > 0 || starts_mid || ends_mid))) {   // (the file may end here; a range may be empty)
                    T.waiting = true;
                    break;
                }
                if (ends_mid) XZ_FAIL(no_end("what starts at byte " + at(pos)));
                if (starts_mid && Z.any_streams == 0) XZ_FAIL(no_start(pos, "stream"));
                if (Z.any_streams == 0 || xz::magic_prefix(p + pos, avail)) XZ_FAIL(xz_fail(c, "stream header at byte " + at(pos), xz::kRanOut));
                XZ_FAIL(xz_fail(c, "at byte " + at(pos), all_zero(p + pos, avail) ? xz::kBadPadding : xz::kTrailing));
            }
            if (!xz::is_magic(p + pos) && starts_mid && Z.any_streams == 0) XZ_FAIL(no_start(pos, "stream"));
            if (!xz::is_magic(p + pos)) XZ_FAIL(xz_fail(c, "at byte " + at(pos), Z.any_streams > 0 && p[pos] == 0 ? xz::kBadPadding : xz::kTrailing));
            const uint32_t hs = xz::stream_header(p + pos, &Z.check);
            if (hs != xz::kOk && starts_mid && Z.any_streams == 0) XZ_FAIL(no_start(pos, "stream"));   // (the magic's bytes, inside some block)
            if (hs != xz::kOk) XZ_FAIL(xz_fail(c, "stream header at byte " + at(pos), hs));
            pos += xz::kHeaderBytes;
            Z.records.clear();
            Z.stage = Stage::Blocks;
            ++Z.any_streams;
            ++stats[WindowPipeline::kXzStreams];
            continue;
        }
        if (avail < 1u) {
            if (ends_mid) {   // (a range may end at a block's first byte: the stitch holds the walker's place against the range's end)
                T.waiting = true;
                break;
            }
            SLIMM_TRY(wait_or("block header at byte " + at(pos)));
            break;
        }
        // (the first thing of a range that starts among a stream's blocks is a block)
        const bool at_start = Z.from_left && T.base + pos == A.range_begin;
        if (p[pos] == 0 && at_start) XZ_FAIL(no_start(pos, "block"));
        if (p[pos] == 0) {   // the index, and the footer behind it
            uint64_t count = 0, first = 0, bytes = 0;
            const std::string where = "index at byte " + at(pos);
            const uint32_t is = xz::index_extent(p + pos, avail, &count, &first, &bytes);
            if (is == xz::kRanOut) {
                SLIMM_TRY(wait_or(where));
                break;
            }
            if (is != xz::kOk) XZ_FAIL(xz_fail(c, where, is));
            if (avail < bytes + xz::kHeaderBytes) {
                SLIMM_TRY(wait_or("stream footer at byte " + at(pos + bytes)));
                break;
            }
            // (of a stream whose header lies on the left the index's last records are this range's blocks; the records in
            // front of them are kept for the stitch, which holds them against the blocks of the ranges on the left)
            const bool open_left = Z.from_left && !Z.left_closed;
            bool same = open_left ? count >= Z.records.size() : count == Z.records.size();
            std::vector<std::pair<uint64_t, uint64_t>> kept;
            for (uint64_t r = 0; same && open_left && r < count - Z.records.size(); ++r) {
                uint64_t unpadded = 0, uncompressed = 0;
                xz::index_record(p + pos, bytes, &first, &unpadded, &uncompressed);
                kept.emplace_back(unpadded, uncompressed);
            }
            for (size_t r = 0; same && r < Z.records.size(); ++r) {
                uint64_t unpadded = 0, uncompressed = 0;
                xz::index_record(p + pos, bytes, &first, &unpadded, &uncompressed);
                same = unpadded == Z.records[r].first && uncompressed == Z.records[r].second;
            }
            if (!same) XZ_FAIL(xz_fail(c, where, xz::kIndexMismatch));
            const uint8_t* foot = p + pos + bytes;
            uint64_t stated = 0;
            if (open_left && foot[9] != Z.check && xz::stream_footer(foot, foot[9], &stated) == xz::kOk)
                XZ_FAIL(fail(c, SLIMM_E_SPLIT, "xz: the stream footer at byte %s states check kind %u, the range was told %u", at(pos + bytes).c_str(),
                             static_cast<unsigned>(foot[9]), static_cast<unsigned>(Z.check)));
            uint32_t fs = xz::stream_footer(foot, Z.check, &stated);
            if (fs == xz::kOk && stated != bytes) fs = xz::kBadFooter;
            if (fs != xz::kOk) XZ_FAIL(xz_fail(c, "stream footer at byte " + at(pos + bytes), fs));
            stats[WindowPipeline::kXzIndexRecords] += count;
            if (open_left) {
                Z.left_kept = std::move(kept);
                Z.left_closed = true;
                Z.left_index_at = T.base + pos;
            }
            Z.records.clear();
            pos += bytes + xz::kHeaderBytes;
            Z.stage = Stage::Between;
            continue;
        }
        // a block: its header, its chunk chain, its padding and check
        const std::string where = "block at byte " + at(pos);
        xz::BlockHeader bh{};
        const uint32_t hs = xz::block_header(p + pos, avail, bh);
        if (hs == xz::kRanOut && !(last && at_start)) {
            SLIMM_TRY(wait_or("block header at byte " + at(pos)));
            break;
        }
        if (hs != xz::kOk && hs != xz::kBadFilter && at_start) XZ_FAIL(no_start(pos, "block"));
        if (hs == xz::kBadFilter) XZ_FAIL(xz_fail(c, "block header at byte " + at(pos), hs, " (filter id " + std::to_string(bh.filter_id) + ")"));
        if (hs != xz::kOk) XZ_FAIL(xz_fail(c, "block header at byte " + at(pos), hs));
        uint64_t q = pos + bh.bytes, btext = 0;
        xz::Rules rules;
        bool whole = false;
        uint32_t bad = xz::kOk;
        for (;;) {
            xz::Chunk ch;
            const uint32_t cs = xz::chunk_header(p + q, n_bytes - q, rules, ch);
            if (cs == xz::kRanOut) break;
            if (cs != xz::kOk) {
                bad = cs;
                break;
            }
            if (ch.control == 0) {
                ++q;
                whole = true;
                break;
            }
            if (n_bytes - q < static_cast<uint64_t>(ch.header) + ch.csize) break;
            btext += ch.usize;
            q += static_cast<uint64_t>(ch.header) + ch.csize;
            if (btext > kXzBlockTextMax) break;
        }
        if (bad != xz::kOk) XZ_FAIL(xz_fail(c, "chunk at byte " + at(q), bad));
        if (btext > kXzBlockTextMax) XZ_FAIL(fail(c, SLIMM_E_INVALID, "an xz block of more than 1 GiB of text: decode this file on the host"));
        const uint64_t comp = q - (pos + bh.bytes), pad = (4u - ((bh.bytes + comp) & 3u)) & 3u, cb = xz::check_bytes(Z.check);
        if (!whole || n_bytes - q < pad + cb) {   // (a block whose bytes are not all at hand waits for the next push)
            SLIMM_TRY(wait_or(where));
            break;
        }
        if (!all_zero(p + q, pad)) XZ_FAIL(xz_fail(c, where, xz::kBadBlockPadding));
        if ((bh.has_compressed && bh.compressed != comp) || (bh.has_uncompressed && bh.uncompressed != btext)) XZ_FAIL(xz_fail(c, where, xz::kBadBlockSizes));
        if (!Z.ready.empty() && text + btext > static_cast<uint64_t>(cap_text)) break;   // (the round is full: this block starts the next one)
        xz::Block b{};
        b.at = pos + bh.bytes, b.end = q, b.text_at = text, b.text_len = btext, b.check_at = q + pad;
        b.dict_size = bh.dict_size, b.check = Z.check, b.piece0 = pieces, b.status = xz::kOk;
        const uint64_t tail = btext % gz::kPiece ? btext % gz::kPiece : (btext ? gz::kPiece : 0u);
        b.last_mul = Z.check == xz::kCheckCrc32 ? gz::crc_x_pow8(tail) : Z.check == xz::kCheckCrc64 ? xz::crc64_x_pow8(tail) : 0u;
        pieces += static_cast<uint32_t>((btext + gz::kPiece - 1u) / gz::kPiece);
        Z.ready.push_back(b);
        Z.ready_at.push_back(T.base + pos);
        Z.records.emplace_back(bh.bytes + comp + cb, btext);
        ++stats[WindowPipeline::kXzBlocks];
        text += btext;
        pos = q + pad + cb;
    }
    Z.text = text;
    return SLIMM_OK;
}

int xz_emit(slimm_ctx* c, uint8_t* dst, uint64_t, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline& W = c->win;
    XF& Z = W.file.xz;
    WindowPipeline::Xz& S = W.xzs;
    hipStream_t st = c->stream;
    uint64_t* stats = W.xz_stats;
    const uint32_t nb = static_cast<uint32_t>(Z.ready.size());
    const uint64_t text = Z.text;
    *n_out = 0;
    if (!nb) return SLIMM_OK;
    const uint64_t drop = W.file.stream.skip_of(text);
    const uint32_t pieces = Z.ready.back().piece0 + static_cast<uint32_t>((Z.ready.back().text_len + gz::kPiece - 1u) / gz::kPiece);
    if (S.text.cap < text + 1u) HIP_TRY(c, S.text.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    if (S.blocks.cap < nb) HIP_TRY(c, S.blocks.ensure_later(nb + (nb >> 2) + 64u, W.outgrown));
    if (S.piece.cap < pieces + 1u) HIP_TRY(c, S.piece.ensure_later(pieces + (pieces >> 3) + 1u, W.outgrown));
    SLIMM_TRY(stream_upload(c, S.comp, kXzTail));
    HIP_TRY(c, hipMemcpyAsync(S.blocks.p, Z.ready.data(), nb * sizeof(xz::Block), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_xz_decode, dim3(nb), dim3(64), 0, st, S.comp.p, W.file.stream.pend.size(), S.blocks.p, nb, S.text.p);
    if (pieces) hipLaunchKernelGGL(k_xz_check, dim3((pieces + 255u) / 256u), dim3(256), 0, st, S.blocks.p, nb, pieces, S.text.p, S.piece.p);
    hipLaunchKernelGGL(k_xz_fold, dim3((nb + 63u) / 64u), dim3(64), 0, st, S.blocks.p, nb, S.piece.p, gz::crc_x_pow8(gz::kPiece), xz::crc64_x_pow8(gz::kPiece));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.blocks.p, nb * sizeof(xz::Block), hipMemcpyDeviceToHost, st));
    if (text > drop) {
        HIP_TRY(c, hipMemcpyAsync(dst, S.text.p + drop, text - drop, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(last_byte, dst + (text - drop) - 1u, 1, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    ++stats[WindowPipeline::kXzRounds];
    const uint8_t* p = W.file.stream.pend.data();
    for (uint32_t k = 0; k < nb; ++k) {
        const xz::Block& b = Z.ready[k];
        const std::string where = "block at byte " + std::to_string(Z.ready_at[k]);
        if (b.status != xz::kOk) return xz_fail(c, where, b.status);
        if (b.check == xz::kCheckCrc32) {
            const uint32_t reg = gz::crc_mul(0xffffffffu, gz::crc_x_pow8(b.text_len)) ^ static_cast<uint32_t>(b.crc);
            if (xz::le32(p + b.check_at) != ~reg) return xz_fail(c, where, xz::kBadCheck);
        } else if (b.check == xz::kCheckCrc64) {
            const uint64_t reg = xz::crc64_mul(~0ull, xz::crc64_x_pow8(b.text_len)) ^ b.crc;
            if (xz::le64(p + b.check_at) != ~reg) return xz_fail(c, where, xz::kBadCheck);
        }
        ++stats[b.check == xz::kCheckCrc32   ? WindowPipeline::kXzCheckCrc32
                : b.check == xz::kCheckCrc64 ? WindowPipeline::kXzCheckCrc64
                : b.check == xz::kCheckSha256 ? WindowPipeline::kXzSha256Unverified
                                              : WindowPipeline::kXzCheckNone];
        stats[WindowPipeline::kXzLzmaChunks] += b.lzma_chunks;
        stats[WindowPipeline::kXzRawChunks] += b.raw_chunks;
        stats[WindowPipeline::kXzStateResets] += b.state_resets;
        stats[WindowPipeline::kXzPropChanges] += b.prop_changes;
        stats[WindowPipeline::kXzOddProps] += b.odd_props;
        stats[WindowPipeline::kXzMatchBytes] += b.match_bytes;
        stats[WindowPipeline::kXzMaxDist] = std::max<uint64_t>(stats[WindowPipeline::kXzMaxDist], b.max_dist);
    }
    stats[WindowPipeline::kXzText] += text;
    *n_out = text - drop;
    push_trace_xz("round %llu: %u blocks -> %.1f MB of text", (unsigned long long)stats[WindowPipeline::kXzRounds], nb, text / 1e6);
    Z.ready.clear();
    Z.text = 0;
    return SLIMM_OK;
}

void xz_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const uint64_t* s = c->win.xz_stats;
    fprintf(stderr, "[push xz] %llu streams, %llu blocks in %llu rounds; chunks: %llu LZMA (%llu state resets, %llu properties bytes), %llu "
                    "uncompressed; checks: %llu none, %llu CRC32, %llu CRC64, %llu SHA-256 not verified; %llu match bytes, longest distance %llu; "
                    "%llu compressed bytes -> %llu bytes of text; %llu index records checked\n",
            (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[13], (unsigned long long)s[2], (unsigned long long)s[4],
            (unsigned long long)s[5], (unsigned long long)s[3], (unsigned long long)s[7], (unsigned long long)s[8], (unsigned long long)s[9],
            (unsigned long long)s[10], (unsigned long long)s[11], (unsigned long long)s[12], (unsigned long long)s[15], (unsigned long long)s[14],
            (unsigned long long)s[16]);
}

}  // namespace slimm
