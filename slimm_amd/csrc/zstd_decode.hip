// zstd-compressed SAM decoded on the device (include/slimm_hip.h: slimm_push_zstd_sam_bytes; the format: zstd_frame.h).
// Every block states its size, so the block chain is a host walk; a block's entropy decode needs nothing of the text in
// front of it; only the copies reach back.  The bytes at hand go through stages, a ROUND:
//   (host)        the plan: frame and block headers walked, whole blocks only; of a compressed block the literals header,
//                 the sequences header and the lengths of its table descriptions read, so that every scratch is sized
//                 exactly; a code or table that a block repeats is copied behind the round's bytes (the one in front may
//                 lie in an earlier round)
//   k_zs_entropy  a wave per compressed block, tables in LDS: lane 0 the Huffman code, lanes 0-3 the literal streams, lanes
//                 0-2 the three FSE tables, lane 0 the sequences -- {where its literals start in the block's text and in
//                 its literals, offset} each.  The repeat offsets in front of the block are not known: the lane works
//                 with "slot i of them, minus k" and leaves the block's three offsets behind it in the same terms
//   (host)        the blocks' offsets in front composed along each frame; the text offsets (a prefix of the blocks' sizes,
//                 each checked against the block maximum, a frame's total against its content size)
//   k_zs_expand   a thread per byte of the round's text: its block and its sequence by binary search; a literal byte is
//                 written, a match byte gets the position it copies from -- in the round, or in the history in front of it
//                 (the frame's last window of text, kept from round to round), else the stream is corrupt
//   k_zs_double   pointer doubling until nothing changes: at most ceil(log2(text + history)) + 1 passes
//   k_zs_gather   the match bytes fetched from where their chains end (both: lz_resolve.hip, shared with lz4_decode.hip)
//   (host)        XXH64 of the frames that state one, on a copy of the round's text, while the device decodes the
//                 window's SAM records (zs_check)
// No workgroup waits for another: ordering comes from kernel boundaries only.
#include "context.h"

namespace slimm {
namespace {

constexpr uint64_t kZsRoundText = 512ull << 20;   // a round's text at most, by the blocks' bounds (SLIMM_FORCE zstd_round_text=N)
using ZF = WindowPipeline::File::Zstd;

__global__ __launch_bounds__(64) void k_zs_entropy(const uint8_t* __restrict__ base, zs::Block* __restrict__ blocks, uint32_t n, uint8_t* __restrict__ lit,
                                                    zs::Seq* __restrict__ seq) {
    __shared__ uint16_t huf[1u << zs::kHufLogMax];
    __shared__ uint32_t fse[512u + 256u + 512u];
    __shared__ uint32_t logs[4], status;
    __shared__ zs::LitStream streams[4];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    zs::Block& b = blocks[i];
    if (b.type != zs::kCompressed) return;
    if (lane == 0) status = zs::kOk;
    __syncthreads();
    if (b.lit_type >= 2u) {
        if (lane == 0) {   // (the weights' own FSE table: in the sequence tables' room, which is not in use yet)
            uint8_t w[256];
            uint32_t n_w = 0, used = 0, log = 0;
            uint32_t st = zs::huf_read_weights(base + b.huf_at, b.huf_len, w, n_w, used, fse);
            if (st == zs::kOk) st = zs::huf_build(w, n_w, huf, log);
            if (st == zs::kOk) st = zs::literal_streams(base, b, streams);
            logs[3] = log;
            status = st;
        }
        __syncthreads();
        if (status == zs::kOk && lane < b.lit_streams) {
            const zs::LitStream s = streams[lane];
            const uint32_t st = zs::huf_decode_stream(base + s.at, s.len, huf, logs[3], lit + b.lit_out + s.out, s.count);
            if (st != zs::kOk) atomicMax(&status, st);
        }
        __syncthreads();
    }
    const bool ok = status == zs::kOk;
    __syncthreads();
    if (b.n_seq && ok) {
        if (lane < 3u) {
            uint32_t log = 0;
            const uint32_t st = zs::seq_table(base, b.table[lane], lane, fse + (lane == 0 ? 0u : lane == 1 ? 512u : 768u), log);
            logs[lane] = log;
            if (st != zs::kOk) atomicMax(&status, st);
        }
        __syncthreads();
        if (lane == 0 && status == zs::kOk) {
            const zs::SeqTables t{{fse, fse + 512, fse + 768}, {logs[0], logs[1], logs[2]}};
            uint32_t rep[3] = {zs::sym(0), zs::sym(1), zs::sym(2)}, regen = 0;
            status = zs::seq_decode(base + b.bits_at, b.bits_len, t, b.n_seq, b.lit_regen, b.max, seq + b.seq_out, rep, regen);
            b.regen = regen;
            b.rep[0] = rep[0], b.rep[1] = rep[1], b.rep[2] = rep[2];
        }
    } else if (lane == 0) {
        seq[b.seq_out] = zs::Seq{0, 0, 0};
        b.regen = b.lit_regen;
        b.rep[0] = zs::sym(0), b.rep[1] = zs::sym(1), b.rep[2] = zs::sym(2);
        if (ok && b.lit_regen > b.max) status = zs::kBlockTooLarge;
    }
    __syncthreads();
    if (lane == 0) b.status = status;
}

// text: [history H | the round's n_text]; src[i]: the position in it that byte H + i is a copy of (itself: a literal)
__global__ __launch_bounds__(256) void k_zs_expand(const uint8_t* __restrict__ base, const zs::Block* __restrict__ blocks, uint32_t n_blocks,
                                                    const uint8_t* __restrict__ lit, const zs::Seq* __restrict__ seq, uint8_t* __restrict__ text,
                                                    uint32_t* __restrict__ src, uint64_t H, uint64_t n_text, unsigned long long* __restrict__ count) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t trips = (n_text + stride - 1u) / stride;   // (every lane of a wave makes them all: the ballots are reached by all)
    uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t t = 0; t < trips; ++t, i += stride) {
        bool front = false, hist = false;
        if (i < n_text) {
            uint32_t lo = 0, hi = n_blocks;   // the last block whose text starts at or in front of i
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (blocks[mid].text_at <= i) lo = mid; else hi = mid;
            }
            const zs::Block& b = blocks[lo];
            const uint32_t k = static_cast<uint32_t>(i - b.text_at);
            const uint32_t self = static_cast<uint32_t>(H + i);
            uint32_t from = self;
            uint8_t v = 0;
            if (b.type == zs::kRaw) v = base[b.at + k];
            else if (b.type == zs::kRleBlock) v = base[b.at];
            else {
                const zs::Seq* s = seq + b.seq_out;
                uint32_t a = 0, z = b.n_seq + 1u;   // the last sequence that starts at or in front of k
                while (z - a > 1u) {
                    const uint32_t mid = (a + z) >> 1;
                    if (s[mid].out <= k) a = mid; else z = mid;
                }
                const uint32_t j = k - s[a].out;
                const uint32_t ll = a < b.n_seq ? s[a + 1u].lit - s[a].lit : b.lit_regen - s[a].lit;
                if (j < ll) {
                    const uint32_t at = s[a].lit + j;
                    v = b.lit_type == 0u ? base[b.lit_at + at] : b.lit_type == 1u ? base[b.lit_at] : lit[b.lit_out + at];
                } else {
                    const uint32_t off = zs::substitute(s[a].off, b.entry);
                    const int64_t to = static_cast<int64_t>(self) - static_cast<int64_t>(off);
                    if (!off || off > b.window || to < b.reach_lo) {
                        atomicAdd(&count[1], 1ull);
                        atomicMin(&count[2], static_cast<unsigned long long>(lo));
                    } else {
                        from = static_cast<uint32_t>(to);
                        front = static_cast<uint64_t>(to) < H + b.text_at;
                        hist = static_cast<uint64_t>(to) < H;
                    }
                }
            }
            if (from == self) text[self] = v;
            src[i] = from;
        }
        const uint64_t mf = __ballot(front), mh = __ballot(hist);
        if ((threadIdx.x & 63u) == 0u) {
            if (mf) atomicAdd(&count[3], static_cast<unsigned long long>(__popcll(mf)));
            if (mh) atomicAdd(&count[4], static_cast<unsigned long long>(__popcll(mh)));
        }
    }
}

void push_trace_zs(const char* fmt, ...) {   // "[push zstd] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("zstd", fmt, ap);
    va_end(ap);
}

// the host reader's words (host/alignment_file.cpp: codec_read)
int zs_fail(slimm_ctx* c, const std::string& where, uint32_t status) {
    return fail(c, SLIMM_E_INVALID, "zstd-compressed input is not supported unless it decodes: %s: %s", where.c_str(), zs::status_text(status));
}

}  // namespace

bool zs_next_window(const slimm_ctx* c, uint64_t, uint64_t* n) {   // (a round's text is one window: kZsRoundText)
    const ZF& Z = c->win.file.zst;
    *n = Z.text - std::min(Z.text, c->win.file.stream.skip_left);
    return !Z.ready.empty();
}

int zs_round(slimm_ctx* c, bool last) {
    WindowPipeline& W = c->win;
    ZF& Z = W.file.zst;
    WindowPipeline::File::Stream& T = W.file.stream;
    WindowPipeline::Zstd& S = W.zst;
    hipStream_t st = c->stream;
    uint64_t* stats = W.zs_stats;
    Z.ready.clear(), Z.ready_at.clear(), Z.frames.clear(), Z.aux.clear();
    Z.text = 0;
    if (T.waiting && !last) return SLIMM_OK;
    T.waiting = false;   // (at the file's end what waited for bytes is looked at again: it ends the frames, or is truncated)
    // (what the rounds so far have read is gone: a round copies to the device only what is still to decode)
    RoundCursor cur(c, W, last, "zstd", "frame", "frame");
    long cap_text = 0;
    if (!forced("zstd_round_text", &cap_text) || cap_text <= 0) cap_text = static_cast<long>(kZsRoundText);
    // ---- the plan: the container's items (zstd_walk.h), whole blocks only
    using Walk = zs::Walker;
    Walk& K = Z.walk;
    const uint64_t aux_base = T.pend.size() + zs::kPad;
    const uint8_t* p = T.pend.data();
    uint64_t bound = 0, lit_bytes = 0, n_seq_slots = 0;
    for (;;) {
        const Walk::Item it = K.peek(cur.p(), cur.avail(), cur.at());
        if (it.kind <= Walk::MayEnd) {   // (no item: an error, or what stands here needs more bytes -- RoundCursor)
            // (a magic that is cut short is "what starts here"; a skippable frame or a frame header cut short is itself)
            const bool between = K.stage == Walk::Between && (it.kind != Walk::More || it.place == zs::Place::At);
            SLIMM_TRY(cur.settle(it.kind == Walk::Error, between, K.frames > 0, it.where(), it.words()));
            break;
        }
        if (it.kind == Walk::SkippableFrame) ++stats[WindowPipeline::kZsSkippable];
        if (it.kind == Walk::Header) {
            Z.frame_len = 0;
            Z.entropy.reset();
            Z.rep[0] = 1, Z.rep[1] = 4, Z.rep[2] = 8;
            Z.xxh.reset();
            if (Z.ready.empty()) Z.hist_len = 0;
            ++stats[WindowPipeline::kZsFrames];
        }
        if (it.kind == Walk::Sum) {
            if (!Z.frames.empty() && Z.frames.back().ends) {   // (its last blocks are of this round: zs_check compares)
                Z.frames.back().has_sum = true;
                Z.frames.back().sum = it.sum;
            } else {
                if (it.sum != static_cast<uint32_t>(Z.xxh.digest())) return zs_fail(c, zs::place_text(zs::Place::Frame, K.frame_at), zs::kBadChecksum);
                ++stats[WindowPipeline::kZsChecksums];
            }
        }
        if (it.kind == Walk::Block) {
            const uint64_t most = it.type == zs::kCompressed ? K.fh.block_max : it.size;
            if (!Z.ready.empty() && bound + most > static_cast<uint64_t>(cap_text)) break;   // (the round is full: this block starts the next one)
            zs::Block b{};
            b.at = cur.pos + 3u, b.size = static_cast<uint32_t>(it.bytes - 3u), b.type = it.type, b.max = K.fh.block_max, b.regen = it.size;
            b.window = static_cast<uint32_t>(K.fh.window);
            b.status = zs::kOk;
            b.rep[0] = zs::sym(0), b.rep[1] = zs::sym(1), b.rep[2] = zs::sym(2);
            if (it.type == zs::kCompressed) {
                const uint32_t ps = zs::plan_compressed(p, b.at, it.size, Z.entropy, Z.aux, aux_base, b, &stats[WindowPipeline::kZsHufTree]);
                if (ps != zs::kOk) return zs_fail(c, it.where(), ps);
                b.lit_out = lit_bytes, b.seq_out = n_seq_slots;
                if (b.lit_type >= 2u) lit_bytes += b.lit_regen;
                n_seq_slots += b.n_seq + 1ull;
                stats[WindowPipeline::kZsSequences] += b.n_seq;
            }
            ++stats[it.type == zs::kRaw ? WindowPipeline::kZsRaw : it.type == zs::kRleBlock ? WindowPipeline::kZsRle : WindowPipeline::kZsCompressed];
            if (Z.frames.empty() || Z.frames.back().ends) {
                ZF::Frame f;
                f.first = static_cast<uint32_t>(Z.ready.size());
                f.fh = K.fh, f.at = K.frame_at, f.len_before = Z.frame_len;
                f.xxh = Z.xxh;   // (what the frame's header set, or what the rounds so far have left)
                for (uint32_t r = 0; r < 3u; ++r) f.rep[r] = Z.rep[r];
                Z.frames.push_back(f);
            }
            b.frame = static_cast<uint32_t>(Z.frames.size() - 1u);
            ++Z.frames.back().n;
            Z.frames.back().ends = it.last;
            Z.ready.push_back(b);
            Z.ready_at.push_back(it.at);
            bound += most;
        }
        K.take(it);
        cur.pos += it.bytes;
    }
    const uint32_t nb = static_cast<uint32_t>(Z.ready.size());
    if (!nb) return SLIMM_OK;
    // ---- the entropy stage
    const uint64_t up = aux_base + Z.aux.size() + zs::kPad;
    if (S.comp.cap < up) HIP_TRY(c, S.comp.ensure_later(up + (up >> 3), W.outgrown));
    if (S.blocks.cap < nb) HIP_TRY(c, S.blocks.ensure_later(nb + (nb >> 2) + 64u, W.outgrown));
    if (S.lit.cap < lit_bytes + 1u) HIP_TRY(c, S.lit.ensure_later(lit_bytes + (lit_bytes >> 3) + 1u, W.outgrown));
    if (S.seq.cap < n_seq_slots + 1u) HIP_TRY(c, S.seq.ensure_later(n_seq_slots + (n_seq_slots >> 3) + 1u, W.outgrown));
    HIP_TRY(c, S.count.ensure(8));
    SLIMM_TRY(stream_upload(c, S.comp, zs::kPad));   // (room for it and for aux: above)
    if (!Z.aux.empty()) HIP_TRY(c, hipMemcpyAsync(S.comp.p + aux_base, Z.aux.data(), Z.aux.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(S.comp.p + aux_base + Z.aux.size(), 0, zs::kPad, st));
    HIP_TRY(c, hipMemcpyAsync(S.blocks.p, Z.ready.data(), nb * sizeof(zs::Block), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_zs_entropy, dim3(nb), dim3(64), 0, st, S.comp.p, S.blocks.p, nb, S.lit.p, S.seq.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.blocks.p, nb * sizeof(zs::Block), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ++stats[WindowPipeline::kZsRounds];
    // ---- the repeat offsets composed, the text offsets
    uint64_t text = 0;
    for (ZF::Frame& f : Z.frames) {
        f.text_at = text;
        uint32_t cur[3] = {f.rep[0], f.rep[1], f.rep[2]};
        for (uint32_t k = f.first; k < f.first + f.n; ++k) {
            zs::Block& b = Z.ready[k];
            const std::string where = "block at byte " + std::to_string(Z.ready_at[k]);
            if (b.status != zs::kOk) return zs_fail(c, where, b.status);
            if (b.regen > b.max) return zs_fail(c, where, zs::kBlockTooLarge);
            for (uint32_t r = 0; r < 3u; ++r) b.entry[r] = cur[r];
            uint32_t out[3];
            for (uint32_t r = 0; r < 3u; ++r) {
                out[r] = zs::substitute(b.rep[r], b.entry);
                if (!out[r]) return zs_fail(c, where, zs::kBadOffset);
            }
            for (uint32_t r = 0; r < 3u; ++r) cur[r] = out[r];
            b.text_at = text;
            text += b.regen;
        }
        f.text_len = text - f.text_at;
        if (f.ends) {
            if (f.fh.has_size && f.fh.content_size != f.len_before + f.text_len)
                return zs_fail(c, "frame at byte " + std::to_string(f.at), zs::kBadContentSize);
        } else {   // (it goes on into the next round -- and is the round's last: no header was read behind it)
            for (uint32_t r = 0; r < 3u; ++r) Z.rep[r] = cur[r];
            Z.frame_len = f.len_before + f.text_len;
        }
    }
    if (text >= (1ull << 31)) return fail(c, SLIMM_E_INVALID, "a round of zstd blocks of 2 GiB of text or more");
    // where a match may reach: the first frame of the round goes on from the history, the others start in the round
    const uint64_t H = Z.hist_len;
    for (uint32_t k = 0; k < nb; ++k) {
        const ZF::Frame& f = Z.frames[Z.ready[k].frame];
        Z.ready[k].reach_lo = f.len_before ? 0 : static_cast<int64_t>(H + f.text_at);
    }
    Z.text = text;
    return SLIMM_OK;
}

int zs_emit(slimm_ctx* c, uint8_t* dst, uint64_t, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline& W = c->win;
    ZF& Z = W.file.zst;
    WindowPipeline::Zstd& S = W.zst;
    hipStream_t st = c->stream;
    uint64_t* stats = W.zs_stats;
    const uint32_t nb = static_cast<uint32_t>(Z.ready.size());
    const uint64_t text = Z.text, H = Z.hist_len;
    *n_out = 0;
    if (!nb) return SLIMM_OK;
    const uint64_t drop = W.file.stream.skip_of(text);
    if (S.text.cap < H + text + 1u) HIP_TRY(c, S.text.ensure_later(H + text + (text >> 3) + 1u, W.outgrown));
    if (S.src.cap < text + 1u) HIP_TRY(c, S.src.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    if (H) HIP_TRY(c, hipMemcpyAsync(S.text.p, S.hist.p, H, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(S.blocks.p, Z.ready.data(), nb * sizeof(zs::Block), hipMemcpyHostToDevice, st));
    unsigned long long count[5] = {0, 0, ~0ull, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(S.count.p, count, sizeof(count), hipMemcpyHostToDevice, st));
    uint32_t passes = 0;
    if (text) {
        hipLaunchKernelGGL(k_zs_expand, dim3(copy_grid_for(text)), dim3(256), 0, st, S.comp.p, S.blocks.p, nb, S.lit.p, S.seq.p, S.text.p, S.src.p, H, text,
                           S.count.p);
        HIP_TRY(c, hipGetLastError());
        SLIMM_TRY(resolve_copies(c, "zstd", S.src.p, S.text.p, H, text, S.count.p, count, &passes));   // (lz_resolve.hip)
        if (count[1]) {
            const uint64_t k = std::min<uint64_t>(count[2], nb - 1u);
            return zs_fail(c, "block at byte " + std::to_string(Z.ready_at[k]), zs::kBadOffset);
        }
    }
    // the history for the next round: the last window of the frame that goes on -- none when the round's last frame ended
    const ZF::Frame& f = Z.frames.back();
    uint64_t keep = 0;
    if (!f.ends) keep = std::min<uint64_t>(f.fh.window, f.len_before + f.text_len);
    if (keep) {
        if (S.hist.cap < keep) HIP_TRY(c, S.hist.ensure_later(std::min<uint64_t>(f.fh.window, 2u * keep), W.outgrown));
        HIP_TRY(c, hipMemcpyAsync(S.hist.p, S.text.p + (H + text - keep), keep, hipMemcpyDeviceToDevice, st));
    }
    if (text > drop) {
        HIP_TRY(c, hipMemcpyAsync(dst, S.text.p + H + drop, text - drop, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(last_byte, dst + (text - drop) - 1u, 1, hipMemcpyDeviceToHost, st));
    }
    // (the frames that state a checksum: their text to the host, for zs_check)
    Z.round_hist = H;
    bool sums = false;
    for (const ZF::Frame& fr : Z.frames) sums = sums || (fr.fh.has_checksum && fr.text_len);
    if (sums) {
        if (S.h_text.cap < text) HIP_TRY(c, S.h_text.ensure(text + (text >> 3)));
        HIP_TRY(c, hipMemcpyAsync(S.h_text.p, S.text.p + H, text, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    stats[WindowPipeline::kZsFromFront] += count[3];
    stats[WindowPipeline::kZsFromHistory] += count[4];
    stats[WindowPipeline::kZsPasses] = std::max<uint64_t>(stats[WindowPipeline::kZsPasses], passes);
    stats[WindowPipeline::kZsText] += text;
    Z.hist_len = keep;
    *n_out = text - drop;
    push_trace_zs("round %llu: %u blocks -> %.1f MB of text, %u passes", (unsigned long long)stats[WindowPipeline::kZsRounds], nb, text / 1e6, passes);
    return SLIMM_OK;
}

int zs_check(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    ZF& Z = W.file.zst;
    for (ZF::Frame& f : Z.frames) {
        if (!f.fh.has_checksum) continue;
        if (f.text_len) f.xxh.update(W.zst.h_text.p + f.text_at, f.text_len);
        if (f.ends && f.has_sum) {
            if (f.sum != static_cast<uint32_t>(f.xxh.digest())) return zs_fail(c, "frame at byte " + std::to_string(f.at), zs::kBadChecksum);
            ++W.zs_stats[WindowPipeline::kZsChecksums];
        } else {   // (the round's last frame: it goes on, or its checksum's bytes have not come yet)
            Z.xxh = f.xxh;
        }
    }
    Z.ready.clear(), Z.frames.clear();
    Z.text = 0;
    return SLIMM_OK;
}

void zs_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const uint64_t* s = c->win.zs_stats;
    fprintf(stderr, "[push zstd] %llu frames (%llu skippable), blocks: %llu raw, %llu RLE, %llu compressed; %llu sequences; %llu match bytes from in "
                    "front of their block (%llu from an earlier round); %llu rounds, at most %llu passes; %llu compressed bytes -> %llu bytes of text; "
                    "%llu checksums checked\n",
            (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3], (unsigned long long)s[4],
            (unsigned long long)s[12], (unsigned long long)s[13], (unsigned long long)s[14], (unsigned long long)s[15], (unsigned long long)s[19],
            (unsigned long long)s[17], (unsigned long long)s[16], (unsigned long long)s[18]);
}

// ---- a file split by byte range over a group's members: this codec's check in slimm_group_stitch_ranges (windows.h)
int split_zstd_ends(slimm_ctx* const* members, uint32_t n, uint32_t* bad) {
    for (uint32_t k = 0; k < n; ++k) {
        slimm_ctx* c = members[k];
        const WindowPipeline::Announced& A = c->win.announced;
        const WindowPipeline::File::Stream& T = c->win.file.stream;
        const uint64_t at = T.base + (T.bit >> 3);   // (the file's byte its decoder stands at)
        *bad = k;
        if (c->win.file.stream.codec != WindowPipeline::File::Codec::Zstd || !A.has_range)
            return fail(c, SLIMM_E_INVALID, "a range of a zstd file: slimm_set_input_range tells where it lies");
        if (c->win.file.zst.walk.stage != zs::Walker::Between || at != A.range_end || T.pend.size() != (T.bit >> 3))
            return fail(c, SLIMM_E_SPLIT, "zstd: the frames of member %u end at byte %llu, its range at byte %llu: the range does not end at a frame boundary", k,
                        static_cast<unsigned long long>(at), static_cast<unsigned long long>(A.range_end));
    }
    return SLIMM_OK;
}

}  // namespace slimm
