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
// an index whose first records are blocks of the ranges on its left (split_xz_streams, below, holds them against those).
// No workgroup waits for another.  One round is one window; the window then goes to the SAM finder and decoder as any text
// window does (windows.hip).  NOT MEASURED on an MI355X: nothing is known of an LZMA lane's rate there.
#include "context.h"

namespace slimm {
namespace {

constexpr uint64_t kXzTail = 16;                    // zeroed bytes behind the compressed bytes on the device
constexpr uint64_t kXzRoundText = 512ull << 20;     // a round's text at most (SLIMM_FORCE xz_round_text=N), or one block alone
constexpr uint64_t kXzBlockTextMax = 1ull << 30;    // one block of more text than that is refused
using XF = WindowPipeline::File::Xz;

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

}  // namespace

void launch_xz_checks(hipStream_t st, xz::Block* blocks, uint32_t n, uint32_t n_pieces, const uint8_t* text, xz::Piece* piece) {
    if (n_pieces) hipLaunchKernelGGL(k_xz_check, dim3((n_pieces + 255u) / 256u), dim3(256), 0, st, blocks, n, n_pieces, text, piece);
    hipLaunchKernelGGL(k_xz_fold, dim3((n + 63u) / 64u), dim3(64), 0, st, blocks, n, piece, gz::crc_x_pow8(gz::kPiece), xz::crc64_x_pow8(gz::kPiece));
}

namespace {

void push_trace_xz(const char* fmt, ...) {   // "[push xz] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("xz", fmt, ap);
    va_end(ap);
}

// the host reader's words (host/alignment_file.cpp: codec_read)
int xz_fail(slimm_ctx* c, const std::string& where, uint32_t status) {
    return fail(c, SLIMM_E_INVALID, "xz-compressed input is not supported unless it decodes: %s: %s", where.c_str(), xz::status_text(status));
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
    // (errors come in file order: what is wrong behind blocks that are ready is looked at again by the next round, once those
    // blocks are decoded -- nothing is read past it: RoundCursor::hold)
    RoundCursor cur(c, W, last, "xz", "stream", "block");
    long cap_text = 0;
    if (!forced("xz_round_text", &cap_text) || cap_text <= 0) cap_text = static_cast<long>(kXzRoundText);
    using Walk = xz::Walker;
    Walk& K = Z.walk;
    const WindowPipeline::Announced& A = W.announced;
    if (!Z.started) {
        Z.started = true;
        if (cur.starts_mid && A.xz_check >= 0) {   // (among the blocks of a stream whose header lies in a range on the left)
            K.among_blocks(static_cast<uint32_t>(A.xz_check));
            Z.from_left = true;
        }
    }
    const uint64_t n_bytes = T.pend.size();
    const uint8_t* p = T.pend.data();
    uint64_t text = 0;
    uint32_t pieces = 0;
    for (;;) {
        const Walk::Item it = K.peek(cur.p(), cur.avail(), cur.at());
        // (the first thing of a range that starts among a stream's blocks is a block)
        const bool at_start = Z.from_left && cur.at() == A.range_begin;
        // (a range may end at a block's first byte: the stitch holds the walker's place against the range's end)
        if (K.stage == Walk::Blocks && cur.avail() == 0 && cur.ends_mid && cur.wait() == SLIMM_OK) break;
        if (at_start && cur.avail() > 0 && (it.place >= xz::Place::Index || (it.kind == Walk::Error && it.status != xz::kBadFilter) || (it.kind == Walk::More && last))) {
            SLIMM_TRY(cur.no_start("block"));
            break;
        }
        if (it.kind == Walk::Error && it.place == xz::Place::Footer && K.open_left) {   // (the walker held the footer against the kind that was told)
            const uint8_t* foot = cur.p() + (it.at - cur.at());
            uint64_t stated = 0;
            if (foot[9] != K.check && xz::stream_footer(foot, foot[9], &stated) == xz::kOk) {
                if (!cur.hold) return fail(c, SLIMM_E_SPLIT, "xz: the stream footer at byte %llu states check kind %u, the range was told %u",
                                           static_cast<unsigned long long>(it.at), static_cast<unsigned>(foot[9]), static_cast<unsigned>(K.check));
                break;
            }
        }
        if (it.kind <= Walk::MayEnd) {   // (no item: an error, or what stands here needs more bytes -- RoundCursor)
            SLIMM_TRY(cur.settle(it.kind == Walk::Error, K.stage == Walk::Between, K.streams > 0, it.where(), it.words()));
            break;
        }
        if (it.kind == Walk::BlockStart) {   // a block: its header, its chunk chain, its padding and check
            const Walk::InBlock before = K.block;
            K.take(it);
            uint64_t q = cur.pos + it.bytes;
            Walk::Item in = K.peek(p + q, n_bytes - q, T.base + q);
            for (; in.kind == Walk::ChunkItem && K.block.text <= kXzBlockTextMax; in = K.peek(p + q, n_bytes - q, T.base + q)) K.take(in), q += in.bytes;
            const uint64_t btext = K.block.text;
            const bool fits = Z.ready.empty() || text + btext <= static_cast<uint64_t>(cap_text);
            if (in.kind != Walk::BlockEnd || btext > kXzBlockTextMax || !fits) {   // (it is left at its header)
                K.leave_block(before);
                if (btext > kXzBlockTextMax) {
                    if (!cur.hold) return fail(c, SLIMM_E_INVALID, "an xz block of more than 1 GiB of text: decode this file on the host");
                } else if (in.kind == Walk::Error) {
                    SLIMM_TRY(cur.fail_words(in.words()));
                } else if (in.kind == Walk::More) {   // (a block whose bytes are not all at hand waits for the next push)
                    const std::string where = xz::place_text(xz::Place::Block, it.at);
                    SLIMM_TRY(cur.wait_or(where, where + ": " + xz::status_text(xz::kRanOut)));
                }
                break;   // (or the round is full: this block starts the next one)
            }
            K.take(in);
            xz::Block b{};
            b.at = cur.pos + it.bytes, b.end = q + 1u, b.text_at = text, b.text_len = btext, b.check_at = q + 1u + in.pad;
            b.dict_size = it.bh.dict_size, b.check = K.check, b.piece0 = pieces, b.status = xz::kOk;
            const uint64_t tail = btext % gz::kPiece ? btext % gz::kPiece : (btext ? gz::kPiece : 0u);
            b.last_mul = K.check == xz::kCheckCrc32 ? gz::crc_x_pow8(tail) : K.check == xz::kCheckCrc64 ? xz::crc64_x_pow8(tail) : 0u;
            pieces += static_cast<uint32_t>((btext + gz::kPiece - 1u) / gz::kPiece);
            Z.ready.push_back(b);
            Z.ready_at.push_back(it.at);
            cur.hold = true;
            ++stats[WindowPipeline::kXzBlocks];
            text += btext;
            cur.pos = q + in.bytes;
            continue;
        }
        if (it.kind == Walk::StreamStart) ++stats[WindowPipeline::kXzStreams];
        if (it.kind == Walk::Index) {
            stats[WindowPipeline::kXzIndexRecords] += it.count;
            if (K.open_left) Z.left_kept = it.kept, Z.left_index_at = cur.at();
        }
        K.take(it);
        cur.pos += it.bytes;
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
    launch_xz_checks(st, S.blocks.p, nb, pieces, S.text.p, S.piece.p);
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

// ---- a file split by byte range over a group's members: this codec's check in slimm_group_stitch_ranges (windows.h)
int split_xz_streams(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
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
        if (c->win.file.stream.codec != WindowPipeline::File::Codec::Xz || !A.has_range) return fail(c, SLIMM_E_INVALID, "a range of an xz file: slimm_set_input_range tells where it lies");
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

}  // namespace slimm
