// lz4-compressed SAM decoded on the device (include/slimm_hip.h: slimm_push_lz4_sam_bytes; the format: lz4_frame.h, the
// container: lz4_walk.h).  Every block states its size, so the block chain is a host walk; a block's sequences need nothing
// of the text in front of it; only the copies reach back -- in a linked frame into the blocks in front.  The bytes at hand
// go through stages, a ROUND, as zstd's do (zstd_decode.hip):
//   (host)        the plan: frame headers (their checksums checked) and block headers walked, whole blocks only, up to the
//                 round's caps; the block checksums over the bytes at hand; every scratch sized by a bound -- a block's text
//                 is at most the block maximum, its sequences at most lz4::seq_bound(size)
//   k_lz4_tokens  a wave per compressed block: all 64 lanes stage the block's bytes through an LDS ring, kLz4Chunk at a time
//                 in 16-byte fetches; lane 0 feeds them to the grammar (lz4::SeqWalk) and gathers the sequences in LDS as
//                 {out, lit, off} -- the literals stay where they are --; the wave writes them 64 at a time and leaves the
//                 block's text length, its sequence count and a status.  No byte outside [at, at + size) is read: a fetch
//                 that would cross either end is made byte by byte, and every way the grammar can run off the block's end
//                 is a status of the machine
//   (host)        the text offsets (a prefix of the blocks' lengths, each checked against the block maximum, a frame's
//                 total against its content size); where a block's matches may reach
//   k_lz4_expand  a thread per byte of the round's text: its block and its sequence by binary search; a literal byte is
//                 read from the compressed block and written, a match byte gets the position it copies from -- in the
//                 round, or in the history in front of it (a linked frame's last 64 KiB, kept from round to round), else
//                 the stream is corrupt.  Stored blocks go straight into the text
//   k_zs_double, k_zs_gather   the copies resolved (lz_resolve.hip: zstd's, the one copy of each)
//   (host)        XXH32 of the frames that state one, on a copy of the round's text, while the device decodes the
//                 window's SAM records (lz4_check)
// No workgroup waits for another: ordering comes from kernel boundaries only.
#include "context.h"

namespace slimm {
namespace {

constexpr uint64_t kLz4RoundText = 512ull << 20;   // a round's text at most, by the blocks' bounds (SLIMM_FORCE lz4_round_text=N): zstd's, a stated default
// k_lz4_tokens: the bytes staged at a time and the ring of two such chunks -- with the 64 + 3 gathered sequences 4.9 KiB of
// LDS a wave, so that LDS (160 KiB a CU) admits the 32 one-wave workgroups a CU can hold.  A stated default, not a measurement
constexpr uint32_t kLz4Chunk = 2048, kLz4Ring = 2u * kLz4Chunk;
constexpr uint32_t kLz4Flush = 64;
using LF = WindowPipeline::File::Lz4;

__global__ __launch_bounds__(64) void k_lz4_tokens(const uint8_t* __restrict__ base, lz4::Block* __restrict__ blocks, uint32_t n, lz4::Seq* __restrict__ seq) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kLz4Ring];
    __shared__ lz4::Seq held[kLz4Flush + 3u];
    __shared__ uint32_t sh_pos, sh_held, sh_done;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    lz4::Block& b = blocks[i];
    if (b.stored) return;
    const uint32_t size = b.size, cap = lz4::seq_bound(size);
    const uint8_t* p = base + b.at;
    // positions are counted from the 16-byte line the block starts in: `a` is its first byte's, chunk k holds [k, k + 1) * kLz4Chunk
    const uint32_t a = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 15u), end = a + size;
    lz4::Seq* out = seq + b.seq_out;
    lz4::SeqWalk w;   // (lane 0's)
    uint32_t staged_lo = 0, staged_hi = 0, written = 0;
    bool over = false;
    if (lane == 0) sh_pos = 0, sh_held = 0, sh_done = 0;
    __syncthreads();
    for (;;) {
        // ---- the ring: the chunk of the byte wanted next and the one behind it, whichever of them it does not hold yet
        const uint32_t c0 = (sh_pos + a) / kLz4Chunk;
        for (uint32_t k = c0; k < c0 + 2u; ++k) {
            if ((k >= staged_lo && k < staged_hi) || k * kLz4Chunk >= end) continue;
            for (uint32_t u = k * kLz4Chunk + lane * 16u; u < (k + 1u) * kLz4Chunk; u += 64u * 16u) {
                uint8_t* d = ring + (u % kLz4Ring);
                if (u >= a && u + 16u <= end) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(p + (u - a));
                else
                    for (uint32_t j = 0; j < 16u; ++j)
                        if (u + j >= a && u + j < end) d[j] = p[u + j - a];
            }
        }
        staged_lo = c0, staged_hi = c0 + 2u;
        __syncthreads();
        // ---- the walk: until the staged bytes are used up, the gathered sequences are a wave's worth, or the block is done
        if (lane == 0) {
            const uint32_t stop = min(staged_hi * kLz4Chunk, end) - a;
            uint32_t h = sh_held;
            while (w.state < lz4::SeqWalk::Done && w.pos < stop && h < kLz4Flush) h += w.step(ring[(w.pos + a) % kLz4Ring], size, held + h);
            if (w.state < lz4::SeqWalk::Done && w.pos >= size) w.fail(w.ran_off());
            sh_pos = w.pos, sh_held = h, sh_done = w.state >= lz4::SeqWalk::Done;
        }
        __syncthreads();
        const uint32_t h = sh_held, done = sh_done;
        if (h >= kLz4Flush || done) {
            for (uint32_t k = lane; k < h; k += 64u) {
                if (written + k < cap) out[written + k] = held[k];
                else over = true;
            }
            written += h;
            __syncthreads();
            if (lane == 0) sh_held = 0;
        }
        if (done) break;
    }
    const bool any_over = __any(over);
    if (lane == 0) {
        const bool ok = w.state == lz4::SeqWalk::Done;
        b.status = !ok ? w.status : any_over ? lz4::kTooManySequences : w.out > b.max ? lz4::kTextTooLarge : lz4::kOk;
        b.text_len = w.out, b.n_seq = ok && written ? written - 1u : 0u, b.n_match = w.matches;
    }
}

// text: [history H | the round's n_text]; src[i]: the position in it that byte H + i is a copy of (itself: a literal)
__global__ __launch_bounds__(256) void k_lz4_expand(const uint8_t* __restrict__ base, const lz4::Block* __restrict__ blocks, uint32_t n_blocks,
                                                     const lz4::Seq* __restrict__ seq, uint8_t* __restrict__ text, uint32_t* __restrict__ src, uint64_t H,
                                                     uint64_t n_text, unsigned long long* __restrict__ count) {
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
            const lz4::Block& b = blocks[lo];
            const uint32_t k = static_cast<uint32_t>(i - b.text_at);
            const uint32_t self = static_cast<uint32_t>(H + i);
            uint32_t from = self;
            uint8_t v = 0;
            if (b.stored) v = base[b.at + k];
            else {
                const lz4::Seq* s = seq + b.seq_out;
                uint32_t a = 0, z = b.n_seq + 1u;   // the last entry that starts at or in front of k (the closing one starts behind it)
                while (z - a > 1u) {
                    const uint32_t mid = (a + z) >> 1;
                    if (s[mid].out <= k) a = mid; else z = mid;
                }
                const lz4::Seq e = s[a];
                const uint32_t j = k - e.out;
                if (e.off == lz4::kLiteralsOnly || j < (e.off >> 16)) v = base[b.at + e.lit + j];
                else {
                    const int64_t to = static_cast<int64_t>(self) - static_cast<int64_t>(e.off & 0xffffu);
                    if (to < b.reach_lo) {
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

void push_trace_lz4(const char* fmt, ...) {   // "[push lz4] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("lz4", fmt, ap);
    va_end(ap);
}

// the host reader's words (host/alignment_file.cpp: codec_read)
int lz4_fail(slimm_ctx* c, const std::string& where, uint32_t status) {
    return fail(c, SLIMM_E_INVALID, "lz4-compressed input is not supported unless it decodes: %s: %s", where.c_str(), lz4::status_text(status));
}

}  // namespace

bool lz4_next_window(const slimm_ctx* c, uint64_t, uint64_t* n) {   // (a round's text is one window: kLz4RoundText)
    const LF& Z = c->win.file.lz;
    *n = Z.text - std::min(Z.text, c->win.file.stream.skip_left);
    return !Z.ready.empty();
}

int lz4_round(slimm_ctx* c, bool last) {
    WindowPipeline& W = c->win;
    LF& Z = W.file.lz;
    WindowPipeline::File::Stream& T = W.file.stream;
    WindowPipeline::Lz4& S = W.lz;
    hipStream_t st = c->stream;
    uint64_t* stats = W.lz_stats;
    Z.ready.clear(), Z.ready_at.clear(), Z.frames.clear();
    Z.text = 0;
    Z.in_round = false;
    if (T.waiting && !last) return SLIMM_OK;
    T.waiting = false;   // (at the file's end what waited for bytes is looked at again: it ends the frames, or is truncated)
    RoundCursor cur(c, W, last, "lz4", "frame", "frame");
    long cap_text = 0;
    if (!forced("lz4_round_text", &cap_text) || cap_text <= 0) cap_text = static_cast<long>(kLz4RoundText);
    // ---- the plan: the container's items (lz4_walk.h), whole blocks only
    using Walk = lz4::Walker;
    Walk& K = Z.walk;
    uint64_t bound = 0, n_seq_slots = 0;
    for (;;) {
        const Walk::Item it = K.peek(cur.p(), cur.avail(), cur.at());
        if (it.kind <= Walk::MayEnd) {   // (no item: an error, or what stands here needs more bytes -- RoundCursor)
            if (it.kind == Walk::Error && !Z.ready.empty()) break;   // (errors come in file order: the blocks in front are decoded first)
            // (a magic that is cut short is "what starts here"; a skippable frame or a frame header cut short is itself)
            const bool between = K.stage == Walk::Between && (it.kind != Walk::More || it.place == lz4::Place::At);
            SLIMM_TRY(cur.settle(it.kind == Walk::Error, between, K.frames > 0, it.where(), it.words()));
            break;
        }
        const std::string frame = lz4::place_text(lz4::Place::Frame, K.frame_at);
        if (it.kind == Walk::SkippableFrame) ++stats[WindowPipeline::kLzSkippable];
        if (it.kind == Walk::Header) {
            Z.frame_len = 0;
            Z.xxh.reset();
            Z.in_round = false;
            if (Z.ready.empty()) Z.hist_len = 0;
            ++stats[WindowPipeline::kLzFrames];
            if (it.fh.linked) ++stats[WindowPipeline::kLzLinked];
        }
        if (it.kind == Walk::EndMark) {
            if (Z.in_round) Z.frames.back().ends = true;   // (its last blocks are of this round: the content size is held against them below)
            else if (K.fh.has_size && K.fh.content_size != Z.frame_len) {
                if (!Z.ready.empty()) break;
                return lz4_fail(c, frame, lz4::kBadContentSize);
            }
        }
        if (it.kind == Walk::Sum) {
            if (Z.in_round) {   // (lz4_check compares)
                Z.frames.back().has_sum = true;
                Z.frames.back().sum = it.sum;
            } else {
                if (it.sum != Z.xxh.digest()) {
                    if (!Z.ready.empty()) break;
                    return lz4_fail(c, frame, lz4::kBadChecksum);
                }
                ++stats[WindowPipeline::kLzContentSums];
            }
        }
        if (it.kind == Walk::Block) {
            const uint64_t most = it.stored ? it.size : K.fh.block_max;
            if (!Z.ready.empty() && bound + most > static_cast<uint64_t>(cap_text)) break;   // (the round is full: this block starts the next one)
            if (K.fh.block_sums) {
                if (it.sum != lz4::xxh32(cur.p() + 4, it.size)) {
                    if (!Z.ready.empty()) break;
                    return lz4_fail(c, it.where(), lz4::kBadBlockChecksum);
                }
                ++stats[WindowPipeline::kLzBlockSums];
            }
            lz4::Block b{};
            b.at = cur.pos + 4u, b.size = it.size, b.stored = it.stored ? 1u : 0u, b.max = K.fh.block_max;
            b.status = lz4::kOk;
            b.text_len = it.stored ? it.size : 0u;
            if (!it.stored) {
                b.seq_out = n_seq_slots;
                n_seq_slots += lz4::seq_bound(it.size);
            }
            ++stats[it.stored ? WindowPipeline::kLzStored : WindowPipeline::kLzCompressed];
            if (!Z.in_round) {
                LF::Frame f;
                f.first = static_cast<uint32_t>(Z.ready.size());
                f.fh = K.fh, f.at = K.frame_at, f.len_before = Z.frame_len;
                f.xxh = Z.xxh;   // (what the frame's header set, or what the rounds so far have left)
                Z.frames.push_back(f);
                Z.in_round = true;
            }
            b.frame = static_cast<uint32_t>(Z.frames.size() - 1u);
            ++Z.frames.back().n;
            Z.ready.push_back(b);
            Z.ready_at.push_back(it.at);
            bound += most;
        }
        K.take(it);
        cur.pos += it.bytes;
    }
    const uint32_t nb = static_cast<uint32_t>(Z.ready.size());
    if (!nb) return SLIMM_OK;
    // ---- the sequences
    if (S.blocks.cap < nb) HIP_TRY(c, S.blocks.ensure_later(nb + (nb >> 2) + 64u, W.outgrown));
    if (S.seq.cap < n_seq_slots + 1u) HIP_TRY(c, S.seq.ensure_later(n_seq_slots + (n_seq_slots >> 3) + 1u, W.outgrown));
    HIP_TRY(c, S.count.ensure(8));
    SLIMM_TRY(stream_upload(c, S.comp, 16));
    HIP_TRY(c, hipMemcpyAsync(S.blocks.p, Z.ready.data(), nb * sizeof(lz4::Block), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lz4_tokens, dim3(nb), dim3(64), 0, st, S.comp.p, S.blocks.p, nb, S.seq.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.blocks.p, nb * sizeof(lz4::Block), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ++stats[WindowPipeline::kLzRounds];
    // ---- the text offsets, the content sizes
    uint64_t text = 0;
    for (LF::Frame& f : Z.frames) {
        f.text_at = text;
        for (uint32_t k = f.first; k < f.first + f.n; ++k) {
            lz4::Block& b = Z.ready[k];
            const std::string where = "block at byte " + std::to_string(Z.ready_at[k]);
            if (b.status != lz4::kOk) return lz4_fail(c, where, b.status);
            if (b.text_len > b.max) return lz4_fail(c, where, lz4::kTextTooLarge);
            stats[WindowPipeline::kLzSequences] += b.stored ? 0u : b.n_match;
            b.text_at = text;
            text += b.text_len;
        }
        f.text_len = text - f.text_at;
        if (f.ends) {
            if (f.fh.has_size && f.fh.content_size != f.len_before + f.text_len) return lz4_fail(c, "frame at byte " + std::to_string(f.at), lz4::kBadContentSize);
        } else {   // (it goes on into the next round -- and is the round's last: no header was read behind it)
            Z.frame_len = f.len_before + f.text_len;
        }
    }
    if (text >= (1ull << 31)) return fail(c, SLIMM_E_INVALID, "a round of lz4 blocks of 2 GiB of text or more");
    // where a match may reach: in an independent frame the block's own first byte; in a linked one 64 KiB in front of it,
    // but not in front of the frame's first byte (the round's first frame goes on from the history, the others start in the round)
    const uint64_t H = Z.hist_len;
    for (uint32_t k = 0; k < nb; ++k) {
        lz4::Block& b = Z.ready[k];
        const LF::Frame& f = Z.frames[b.frame];
        const int64_t own = static_cast<int64_t>(H + b.text_at), frame_lo = f.len_before ? 0 : static_cast<int64_t>(H + f.text_at);
        b.reach_lo = f.fh.linked ? std::max<int64_t>(frame_lo, own - static_cast<int64_t>(lz4::kHistory)) : own;
    }
    Z.text = text;
    return SLIMM_OK;
}

int lz4_emit(slimm_ctx* c, uint8_t* dst, uint64_t, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline& W = c->win;
    LF& Z = W.file.lz;
    WindowPipeline::Lz4& S = W.lz;
    hipStream_t st = c->stream;
    uint64_t* stats = W.lz_stats;
    const uint32_t nb = static_cast<uint32_t>(Z.ready.size());
    const uint64_t text = Z.text, H = Z.hist_len;
    *n_out = 0;
    if (!nb) return SLIMM_OK;
    const uint64_t drop = W.file.stream.skip_of(text);
    if (S.text.cap < H + text + 1u) HIP_TRY(c, S.text.ensure_later(H + text + (text >> 3) + 1u, W.outgrown));
    if (S.src.cap < text + 1u) HIP_TRY(c, S.src.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    if (H) HIP_TRY(c, hipMemcpyAsync(S.text.p, S.hist.p, H, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(S.blocks.p, Z.ready.data(), nb * sizeof(lz4::Block), hipMemcpyHostToDevice, st));
    unsigned long long count[5] = {0, 0, ~0ull, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(S.count.p, count, sizeof(count), hipMemcpyHostToDevice, st));
    uint32_t passes = 0;
    if (text) {
        hipLaunchKernelGGL(k_lz4_expand, dim3(copy_grid_for(text)), dim3(256), 0, st, S.comp.p, S.blocks.p, nb, S.seq.p, S.text.p, S.src.p, H, text, S.count.p);
        HIP_TRY(c, hipGetLastError());
        SLIMM_TRY(resolve_copies(c, "lz4", S.src.p, S.text.p, H, text, S.count.p, count, &passes));   // (lz_resolve.hip)
        if (count[1]) {
            const uint64_t k = std::min<uint64_t>(count[2], nb - 1u);
            return lz4_fail(c, "block at byte " + std::to_string(Z.ready_at[k]), lz4::kBadOffset);
        }
    }
    // the history for the next round: the last 64 KiB of the linked frame that goes on -- none when the round's last frame
    // ended (a frame whose end mark has not come yet goes on too)
    const LF::Frame& f = Z.frames.back();
    uint64_t keep = 0;
    if (!f.ends && f.fh.linked) keep = std::min<uint64_t>(lz4::kHistory, f.len_before + f.text_len);
    if (keep) {
        if (S.hist.cap < keep) HIP_TRY(c, S.hist.ensure_later(lz4::kHistory, W.outgrown));
        HIP_TRY(c, hipMemcpyAsync(S.hist.p, S.text.p + (H + text - keep), keep, hipMemcpyDeviceToDevice, st));
    }
    if (text > drop) {
        HIP_TRY(c, hipMemcpyAsync(dst, S.text.p + H + drop, text - drop, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(last_byte, dst + (text - drop) - 1u, 1, hipMemcpyDeviceToHost, st));
    }
    // (the frames that state a checksum: their text to the host, for lz4_check)
    bool sums = false;
    for (const LF::Frame& fr : Z.frames) sums = sums || (fr.fh.has_checksum && fr.text_len);
    if (sums) {
        if (S.h_text.cap < text) HIP_TRY(c, S.h_text.ensure(text + (text >> 3)));
        HIP_TRY(c, hipMemcpyAsync(S.h_text.p, S.text.p + H, text, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    stats[WindowPipeline::kLzFromFront] += count[3];
    stats[WindowPipeline::kLzFromHistory] += count[4];
    stats[WindowPipeline::kLzPasses] = std::max<uint64_t>(stats[WindowPipeline::kLzPasses], passes);
    stats[WindowPipeline::kLzText] += text;
    Z.hist_len = keep;
    *n_out = text - drop;
    push_trace_lz4("round %llu: %u blocks -> %.1f MB of text, %u passes", (unsigned long long)stats[WindowPipeline::kLzRounds], nb, text / 1e6, passes);
    return SLIMM_OK;
}

int lz4_check(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    LF& Z = W.file.lz;
    for (LF::Frame& f : Z.frames) {
        if (!f.fh.has_checksum) continue;
        if (f.text_len) f.xxh.update(W.lz.h_text.p + f.text_at, f.text_len);
        if (f.ends && f.has_sum) {
            if (f.sum != f.xxh.digest()) return lz4_fail(c, "frame at byte " + std::to_string(f.at), lz4::kBadChecksum);
            ++W.lz_stats[WindowPipeline::kLzContentSums];
        } else {   // (the round's last frame: it goes on, or its checksum's bytes have not come yet)
            Z.xxh = f.xxh;
        }
    }
    Z.ready.clear(), Z.frames.clear();
    Z.text = 0;
    Z.in_round = false;
    return SLIMM_OK;
}

void lz4_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const uint64_t* s = c->win.lz_stats;
    fprintf(stderr, "[push lz4] %llu frames (%llu skippable, %llu linked), blocks: %llu stored, %llu compressed; %llu sequences; %llu match bytes from in "
                    "front of their block (%llu from an earlier round); %llu rounds, at most %llu passes; %llu compressed bytes -> %llu bytes of text; "
                    "%llu block checksums and %llu content checksums checked\n",
            (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3], (unsigned long long)s[4],
            (unsigned long long)s[5], (unsigned long long)s[6], (unsigned long long)s[7], (unsigned long long)s[8], (unsigned long long)s[13],
            (unsigned long long)s[10], (unsigned long long)s[9], (unsigned long long)s[11], (unsigned long long)s[12]);
}

}  // namespace slimm
