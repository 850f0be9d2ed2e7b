// gzip-compressed SAM inflated on the device (include/slimm_hip.h: slimm_push_gzip_sam_bytes; the format: deflate_stream.h).
// A deflate stream has no marks to cut it at, and a block copies from the 32 768 bytes in front of it; so the bytes at
// hand go through stages, a ROUND:
//   k_gz_find     every bit offset: the 17 header bits and the code-length code of a non-final dynamic block that zlib
//                 would take?  Compacted by ballot; k_gz_check then reads the two codes of each (a lane each, tables in
//                 LDS).  What passes is a CANDIDATE; none is trusted
//   (host)        chunk starts: the exact start (behind a member header the host has read, or where the round before
//                 stopped) and the first candidate at or behind every kGzipChunk compressed bytes
//   k_gz_walk     the size pass, a wave's first lane per chunk start: Huffman codes only, text bytes counted, up to the first block
//                 boundary that is a later chunk start, a final block's end, or the end of the bytes (then: the last whole
//                 block boundary passed)
//   (host)        the chain: from the exact start, a chunk is real iff the walk of the one in front ended on its first
//                 bit; the rest is dropped, whatever its walk found
//   k_gz_decode   a wave's first lane per chunk of the chain: decoded again into 16 bits per byte of text, a byte or a marker for a
//                 byte of the 32 768 in front of the chunk (a copy of a marker is that marker)
//   k_gz_windows  one workgroup, chunk by chunk in chain order -- the one serial step --: the last 32 768 bytes of chunk k
//                 resolved from those of chunk k - 1
//   k_gz_resolve  a thread per kPiece bytes of text: markers replaced from the window in front, the bytes into the window
//                 buffer, the piece's CRC register; k_gz_fold sums the pieces of a chunk, the host the chunks of a member
//                 (deflate_stream.h: crc_mul), against the trailer's CRC32 and ISIZE
// What the pipeline keeps from round to round: the last chunk's 32 768 bytes (slot 0 of the window scratch), the bytes from
// the last whole block boundary on, the member's CRC register and length.  The window then goes to the SAM finder and
// decoder as any text window does (windows.hip).
#include "context.h"

namespace slimm {
namespace {

constexpr uint64_t kGzTail = 16;                   // zeroed bytes behind the compressed bytes on the device
constexpr uint64_t kGzipChunk = 64ull << 10;       // compressed bytes between two chunk starts (SLIMM_FORCE gzip_chunk=N)
// Text: the size pass stops a chunk at the first block boundary behind kChunkTextSoft bytes (one lane, one chunk: a stream of
// stored or fixed blocks has no candidates at all); a round decodes chunks of at most kRoundText together -- a chunk
// alone when it is larger, up to kChunkTextMax: one block of more text than that is refused, not guessed at
constexpr uint64_t kChunkTextSoft = 64ull << 20, kRoundText = 512ull << 20, kChunkTextMax = 1ull << 30;
// (a decoder is ONE lane of a wave of its own, tables in LDS, as k_bz2_decode's: lanes of one wave that decode different
// chunks would take each other's branches in turn, and a round has far fewer chunks than the device has waves)

using Stage = WindowPipeline::File::Gzip::Stage;

__global__ __launch_bounds__(256) void k_gz_find(const uint8_t* __restrict__ b, uint64_t n_bytes, uint64_t bit_lo,
                                                  unsigned long long* __restrict__ cand, uint32_t* __restrict__ count, uint32_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t bit_hi = n_bytes * 8u;
    // (every lane of a wave makes the same number of trips: the ballot is reached by all)
    const uint64_t trips = (bit_hi - bit_lo + stride - 1u) / stride;
    uint64_t bit = bit_lo + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t t = 0; t < trips; ++t, bit += stride) {
        const bool hit = bit < bit_hi && gz::cheap_candidate(b, bit, n_bytes);
        const uint64_t m = __ballot(hit);
        if (!m) continue;
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t lead = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(m))) - 1u;
        uint32_t at = 0;
        if (lane == lead) at = atomicAdd(count, static_cast<uint32_t>(__popcll(m)));
        at = __shfl(at, static_cast<int>(lead));
        if (hit) {
            at += static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
            if (at < cap) cand[at] = bit;
        }
    }
}

__global__ __launch_bounds__(64) void k_gz_check(const uint8_t* __restrict__ b, uint64_t n_bytes, const unsigned long long* __restrict__ cand,
                                                      uint32_t n, uint32_t* __restrict__ flag) {
    __shared__ gz::Tables t;
    const uint32_t i = blockIdx.x;
    if (threadIdx.x != 0 || i >= n) return;
    flag[i] = gz::is_candidate(b, cand[i], n_bytes, t) ? 1u : 0u;
}

// is `bit` one of starts[from, n)?  (sorted)
__device__ bool is_start(const unsigned long long* starts, uint32_t from, uint32_t n, uint64_t bit) {
    uint32_t lo = from, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] < bit) lo = mid + 1u; else hi = mid;
    }
    return lo < n && starts[lo] == bit;
}

__global__ __launch_bounds__(64) void k_gz_walk(const uint8_t* __restrict__ b, uint64_t n_bytes, const unsigned long long* __restrict__ starts,
                                                     uint32_t n, uint64_t soft, uint64_t stop_bit, gz::Walk* __restrict__ walk) {
    __shared__ gz::Tables t;
    const uint32_t i = blockIdx.x;
    if (threadIdx.x != 0 || i >= n) return;
    gz::Bits br(b, starts[i], n_bytes);
    gz::Count out;
    gz::Walk w{starts[i], 0, gz::kOk, 0};
    for (;;) {
        bool fin = false;
        const uint32_t st = gz::inflate_block(br, t, out, &fin, nullptr);
        if (st != gz::kOk) {   // (kRanOut: end_bit and n are those of the last whole block boundary)
            w.status = st;
            break;
        }
        w.end_bit = br.pos();
        w.n = out.n;
        w.final = fin ? 1u : 0u;
        // (stop_bit: the end of a byte range of a split file -- a walk that reaches or steps over it goes no further)
        if (fin || out.n >= soft || w.end_bit >= stop_bit || is_start(starts, i + 1u, n, w.end_bit)) break;
    }
    walk[i] = w;
}

__global__ __launch_bounds__(64) void k_gz_decode(const uint8_t* __restrict__ b, uint64_t n_bytes, gz::Chunk* __restrict__ chunks, uint32_t n,
                                                       uint16_t* __restrict__ sym) {
    __shared__ gz::Tables t;
    const uint32_t i = blockIdx.x;
    if (threadIdx.x != 0 || i >= n) return;
    gz::Chunk& c = chunks[i];
    // (the bytes at hand end where the chunk does: a block that would read past it has run out)
    gz::Bits br(b, c.start_bit, (c.stop_bit + 7u) >> 3 < n_bytes ? (c.stop_bit + 7u) >> 3 : n_bytes);
    gz::Out16 out{sym + c.text_at, 0, c.len, c.avail};
    uint32_t kinds[3] = {0, 0, 0}, status = gz::kOk;
    while (br.pos() < c.stop_bit) {
        bool fin = false;
        status = gz::inflate_block(br, t, out, &fin, kinds);
        if (status != gz::kOk || fin) break;
    }
    if (status == gz::kOk && (br.pos() != c.stop_bit || out.n != c.len)) status = gz::kOverrun;
    c.status = status;
    for (uint32_t k = 0; k < 3; ++k) c.kinds[k] = kinds[k];
}

// win: slot k + 1 = the last 32 768 bytes of the text up to chunk k's end; slot 0: those in front of chunk 0
__global__ __launch_bounds__(1024) void k_gz_windows(const gz::Chunk* __restrict__ chunks, uint32_t n, const uint16_t* __restrict__ sym,
                                                      uint8_t* __restrict__ win) {
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t* prev = win + static_cast<uint64_t>(k) * gz::kWindow;
        uint8_t* mine = win + static_cast<uint64_t>(k + 1u) * gz::kWindow;
        const uint64_t len = chunks[k].len;
        const uint16_t* s = sym + chunks[k].text_at;
        for (uint32_t i = threadIdx.x; i < gz::kWindow; i += blockDim.x) {
            uint8_t v;
            if (len >= gz::kWindow || i >= gz::kWindow - len) {
                const uint16_t u = s[len - (gz::kWindow - i)];
                v = (u & gz::kMarker) ? prev[u & (gz::kWindow - 1u)] : static_cast<uint8_t>(u);
            } else {
                v = prev[i + len];
            }
            mine[i] = v;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// The window pass of a byte range of a split file (slimm_set_gzip_window_pass): k_gz_windows in 16 bits.  A symbol is a byte,
// or a marker for a byte of the 32 768 in front of the RANGE, which its left neighbour knows; slot 0 before the range's
// first chunk (identity): marker i for byte i.  One workgroup, chunk by chunk
__global__ __launch_bounds__(1024) void k_gz_windows16(const gz::Chunk* __restrict__ chunks, uint32_t n, const uint16_t* __restrict__ sym,
                                                        uint16_t* __restrict__ win, uint32_t identity) {
    if (identity) {
        for (uint32_t i = threadIdx.x; i < gz::kWindow; i += blockDim.x) win[i] = static_cast<uint16_t>(gz::kMarker | i);
        __threadfence_block();
        __syncthreads();
    }
    for (uint32_t k = 0; k < n; ++k) {
        const uint16_t* prev = win + static_cast<uint64_t>(k) * gz::kWindow;
        uint16_t* mine = win + static_cast<uint64_t>(k + 1u) * gz::kWindow;
        const uint64_t len = chunks[k].len;
        const uint16_t* s = sym + chunks[k].text_at;
        for (uint32_t i = threadIdx.x; i < gz::kWindow; i += blockDim.x) {
            uint16_t v;
            if (len >= gz::kWindow || i >= gz::kWindow - len) {
                const uint16_t u = s[len - (gz::kWindow - i)];
                v = (u & gz::kMarker) ? prev[u & (gz::kWindow - 1u)] : u;
            } else {
                v = prev[i + len];
            }
            mine[i] = v;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// a range's final 16-bit window against the 32 768 bytes in front of the range: the bytes in front of the NEXT range
__global__ __launch_bounds__(256) void k_gz_window_apply(const uint16_t* __restrict__ win16, const uint8_t* __restrict__ front, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gz::kWindow) return;
    const uint16_t u = win16[i];
    out[i] = (u & gz::kMarker) ? front[u & (gz::kWindow - 1u)] : static_cast<uint8_t>(u);
}

__global__ __launch_bounds__(256) void k_gz_resolve(const gz::Chunk* __restrict__ chunks, uint32_t n, uint32_t n_pieces, const uint16_t* __restrict__ sym,
                                                     const uint8_t* __restrict__ win, uint64_t drop, uint8_t* __restrict__ dst, uint2* __restrict__ piece) {
    __shared__ uint32_t tab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) tab[i] = gz::crc_table_entry(i);
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    uint32_t lo = 0, hi = n;   // the chunk of piece p: the last one whose piece0 <= p
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (chunks[mid].piece0 <= p) lo = mid; else hi = mid;
    }
    const gz::Chunk& c = chunks[lo];
    const uint64_t from = static_cast<uint64_t>(p - c.piece0) * gz::kPiece;
    const uint64_t to = from + gz::kPiece < c.len ? from + gz::kPiece : c.len;
    const uint8_t* prev = win + static_cast<uint64_t>(lo) * gz::kWindow;
    uint32_t crc = 0, markers = 0;
    for (uint64_t j = from; j < to; ++j) {
        const uint16_t u = sym[c.text_at + j];
        uint8_t v = static_cast<uint8_t>(u);
        if (u & gz::kMarker) {
            v = prev[u & (gz::kWindow - 1u)];
            ++markers;
        }
        crc = tab[(crc ^ v) & 0xffu] ^ (crc >> 8);
        if (c.text_at + j >= drop) dst[c.text_at + j - drop] = v;
    }
    piece[p] = make_uint2(crc, markers);
}

__global__ __launch_bounds__(64) void k_gz_fold(gz::Chunk* __restrict__ chunks, uint32_t n, const uint2* __restrict__ piece, uint32_t full_mul) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gz::Chunk& c = chunks[i];
    const uint32_t np = static_cast<uint32_t>((c.len + gz::kPiece - 1u) / gz::kPiece);
    uint32_t crc = 0;
    uint64_t markers = 0;
    for (uint32_t j = 0; j < np; ++j) {
        const uint2 v = piece[c.piece0 + j];
        crc = gz::crc_mul(crc, j + 1u == np ? c.last_mul : full_mul) ^ v.x;
        markers += v.y;
    }
    c.crc = crc;
    c.markers = markers;
}

void push_trace_gz(const char* fmt, ...) {   // "[push gzip] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("gzip", fmt, ap);
    va_end(ap);
}

#define GZ_CORRUPT(fmt, ...) fail(c, SLIMM_E_INVALID, "corrupt gzip stream (" fmt ")", __VA_ARGS__)
#define GZ_TRUNCATED() fail(c, SLIMM_E_INVALID, "truncated gzip stream")

// A byte range of a split file (slimm_set_gzip_range).  Its end as a bit of the bytes at hand; ~0: the file's end
constexpr uint64_t kNoStop = ~0ull;
uint64_t gz_stop_bit(const slimm_ctx* c) {
    const WindowPipeline::Announced& A = c->win.announced;
    return A.gz_range && A.ends_mid ? A.gz_end_bit - c->win.file.stream.base * 8u : kNoStop;
}
// the bytes ended, or the chain stopped, in front of the range's end: the cut is refused, no verdict on the file
int gz_short_of_end(slimm_ctx* c) {
    const WindowPipeline::File::Stream& T = c->win.file.stream;
    return fail(c, SLIMM_E_SPLIT, "gzip: the chain of the range stands at bit %llu behind its last byte and has not reached the range's end, bit %llu",
                static_cast<unsigned long long>(T.base * 8u + T.bit), static_cast<unsigned long long>(c->win.announced.gz_end_bit));
}
// an error among the blocks: a range that started among a member's blocks may have started where no block does
int gz_bad_blocks(slimm_ctx* c, uint32_t status) {
    if (c->win.file.gz.partial)
        return fail(c, SLIMM_E_SPLIT, "gzip: the blocks from bit %llu on, where the range starts, do not decode (%s)",
                    static_cast<unsigned long long>(c->win.announced.gz_begin_bit), gz::status_text(status));
    return GZ_CORRUPT("%s", gz::status_text(status));
}

// the block candidates of pend from T.bit on, in order; the bytes go to the device first
int gz_find(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    WindowPipeline::File::Stream& T = W.file.stream;
    WindowPipeline::Gzip& S = W.gz;
    hipStream_t st = c->stream;
    const uint64_t n = T.pend.size();
    SLIMM_TRY(stream_upload(c, S.comp, kGzTail));
    HIP_TRY(c, S.count.ensure(4));
    T.cand.clear();
    const uint64_t bits = n * 8u > T.bit ? n * 8u - T.bit : 0u;
    uint32_t got = 0;
    if (bits)
        SLIMM_TRY(stream_candidates(c, S.d_cand, S.count, static_cast<uint32_t>(std::min<uint64_t>(bits / 256u + 1024u, 1u << 27)), [&](uint32_t cap) {
            const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>((bits + 255u) / 256u, 8192u)));
            hipLaunchKernelGGL(k_gz_find, dim3(grid), dim3(256), 0, st, S.comp.p, n, T.bit, S.d_cand.p, S.count.p, cap);
        }, &got));
    if (got) {
        if (S.flag.cap < got) HIP_TRY(c, S.flag.ensure_later(got + (got >> 2), W.outgrown));
        hipLaunchKernelGGL(k_gz_check, dim3(got), dim3(64), 0, st, S.comp.p, n, S.d_cand.p, got, S.flag.p);
        HIP_TRY(c, hipGetLastError());
        std::vector<uint64_t> pre(got);
        std::vector<uint32_t> ok(got);
        HIP_TRY(c, hipMemcpyAsync(pre.data(), S.d_cand.p, got * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(ok.data(), S.flag.p, got * 4u, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < got; ++i)
            if (ok[i]) T.cand.push_back(pre[i]);
    }
    std::sort(T.cand.begin(), T.cand.end());
    W.gz_stats[WindowPipeline::kGzCandidates] += T.cand.size();
    T.found = true;
    return SLIMM_OK;
}

}  // namespace

bool gz_next_window(const slimm_ctx* c, uint64_t, uint64_t* n) {   // (a round's text is one window: kRoundText)
    uint64_t text = 0;
    for (const gz::Chunk& k : c->win.file.gz.ready) text += k.len;
    *n = c->win.file.gz.window_pass ? 0u : text - std::min(text, c->win.file.stream.skip_left);   // (the window pass writes no text)
    return !c->win.file.gz.ready.empty();
}

int gz_round(slimm_ctx* c, bool last) {
    WindowPipeline& W = c->win;
    WindowPipeline::File::Gzip& Z = W.file.gz;
    WindowPipeline::File::Stream& T = W.file.stream;
    WindowPipeline::Gzip& S = W.gz;
    hipStream_t st = c->stream;
    uint64_t* stats = W.gz_stats;
    Z.ready.clear();
    const uint64_t stop = gz_stop_bit(c);
    const bool ends_mid = stop != kNoStop;
    if (Z.range_done) return SLIMM_OK;
    if (W.announced.gz_range && (T.bit == stop || W.announced.gz_begin_bit == W.announced.gz_end_bit)) {   // (the chain stands on the range's end; an empty range)
        Z.range_done = true;
        return SLIMM_OK;
    }
    if (T.waiting && !last) return SLIMM_OK;
    // the candidates in [from, to) of the bytes at hand lie in a trailer or a member header: passed over
    auto pass_over = [&](uint64_t from, uint64_t to) {
        if (!T.found) return;
        stats[WindowPipeline::kGzDropped] += static_cast<uint64_t>(std::lower_bound(T.cand.begin(), T.cand.end(), to) -
                                                                   std::lower_bound(T.cand.begin(), T.cand.end(), from));
    };
    // ---- between the deflate streams, on the host: a trailer, a member header
    while (Z.stage != Stage::Deflate) {
        const uint64_t byte = (T.bit + 7u) >> 3, avail = T.pend.size() - std::min<uint64_t>(byte, T.pend.size());
        const uint8_t* p = T.pend.data() + byte;
        if (Z.stage == Stage::Trailer) {
            if (avail < 8 || (byte + 8u) * 8u > stop) {
                if (last || avail >= 8) return ends_mid ? gz_short_of_end(c) : GZ_TRUNCATED();
                T.waiting = true;
                return SLIMM_OK;
            }
            const uint32_t crc = p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24);
            const uint32_t isize = p[4] | (p[5] << 8) | (p[6] << 16) | (static_cast<uint32_t>(p[7]) << 24);
            if (Z.partial) {   // (the member started in front of the range: the stitch holds its parts against this trailer)
                Z.left = {true, Z.crc, crc, isize, Z.len, T.base + byte};
                Z.partial = false;
            } else if (!Z.window_pass) {
                if (crc != ~Z.crc) return GZ_CORRUPT("%s", gz::status_text(gz::kBadCrc));
                if (isize != static_cast<uint32_t>(Z.len)) return GZ_CORRUPT("%s", gz::status_text(gz::kBadLength));
            }
            pass_over(T.bit, (byte + 8u) * 8u);
            T.bit = (byte + 8u) * 8u;
            Z.stage = Stage::Header;
            ++stats[WindowPipeline::kGzMembers];
            continue;
        }
        if (T.bit == stop) {   // (the range ends between two members)
            Z.range_done = true;
            return SLIMM_OK;
        }
        if (avail == 0) {   // the file is used up between two members
            if (last && ends_mid) return gz_short_of_end(c);
            if (last && stats[WindowPipeline::kGzMembers] == 0) return GZ_TRUNCATED();
            T.waiting = true;
            return SLIMM_OK;
        }
        const long h = gz::member_header(p, avail);
        if (h < 0) return GZ_CORRUPT("%s", "incorrect header check");
        if (h == 0 || (byte + static_cast<uint64_t>(h)) * 8u > stop) {
            if (last || h > 0) return ends_mid ? gz_short_of_end(c) : GZ_TRUNCATED();
            T.waiting = true;
            return SLIMM_OK;
        }
        pass_over(T.bit, (byte + static_cast<uint64_t>(h)) * 8u);
        T.bit = (byte + static_cast<uint64_t>(h)) * 8u;
        Z.stage = Stage::Deflate;
        Z.crc = 0xffffffffu;
        Z.len = 0;
        Z.front = 0;
    }
    if (T.bit == stop) {   // (the range ends right behind a member header: the member's blocks are the next range's)
        Z.range_done = true;
        return SLIMM_OK;
    }
    // ---- a round on the device: candidates, chunk starts, the size pass
    if (!T.found) SLIMM_TRY(gz_find(c));
    const uint64_t n_bytes = T.pend.size(), end_bit = n_bytes * 8u;
    long chunk = 0, every = 0;
    if (!forced("gzip_chunk", &chunk) || chunk <= 0) chunk = static_cast<long>(kGzipChunk);
    std::vector<uint64_t> starts{T.bit};
    const uint64_t cb = static_cast<uint64_t>(chunk) * 8u;
    for (uint64_t target = T.bit + cb;;) {   // (the first candidate at or behind every cb bits)
        const auto it = std::lower_bound(T.cand.begin(), T.cand.end(), target);
        if (it == T.cand.end() || *it >= stop) break;   // (no chunk starts at or behind the range's end)
        starts.push_back(*it);
        target = T.bit + ((*it - T.bit) / cb + 1u) * cb;
    }
    if (forced("gzip_false_starts", &every)) {
        // (tests: chunk starts that start no block -- a few bits into every candidate, and every `every` bits, 4096 by
        // default -- must be walked and dropped without changing anything)
        const uint64_t step = every > 1 ? static_cast<uint64_t>(every) : 4096u;
        const size_t before = starts.size();
        for (auto it = std::upper_bound(T.cand.begin(), T.cand.end(), T.bit); it != T.cand.end(); ++it)
            if (*it + 13u < end_bit) starts.push_back(*it + 13u);
        for (uint64_t b = T.bit + 5u; b + 3u <= end_bit; b += step) starts.push_back(b);
        stats[WindowPipeline::kGzForced] += starts.size() - before;
    }
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    starts.erase(std::lower_bound(starts.begin() + 1, starts.end(), stop), starts.end());
    const uint32_t ns = static_cast<uint32_t>(starts.size());
    if (S.d_cand.cap < ns) HIP_TRY(c, S.d_cand.ensure_later(ns + (ns >> 2) + 256u, W.outgrown));
    if (S.walk.cap < ns) HIP_TRY(c, S.walk.ensure_later(ns + (ns >> 2) + 256u, W.outgrown));
    HIP_TRY(c, hipMemcpyAsync(S.d_cand.p, starts.data(), ns * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_walk, dim3(ns), dim3(64), 0, st, S.comp.p, n_bytes, S.d_cand.p, ns, kChunkTextSoft, stop, S.walk.p);
    HIP_TRY(c, hipGetLastError());
    std::vector<gz::Walk> walk(ns);
    HIP_TRY(c, hipMemcpyAsync(walk.data(), S.walk.p, ns * sizeof(gz::Walk), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ++stats[WindowPipeline::kGzRounds];
    // ---- the chain
    uint64_t cur = T.bit, text = 0, member_len = Z.len;
    size_t i = 0;
    uint32_t pieces = 0;
    bool final = false;
    for (;;) {
        const gz::Walk& w = walk[i];
        if (w.status != gz::kOk && w.status != gz::kRanOut) return gz_bad_blocks(c, w.status);
        if (w.end_bit > cur) {
            if (w.n > kChunkTextMax)
                return fail(c, SLIMM_E_INVALID, "a deflate block of more than 1 GiB of text: decode this file on the host");
            if (!Z.ready.empty() && text + w.n > kRoundText) break;   // (the round is full: this chunk starts the next one)
            gz::Chunk k{};
            k.start_bit = cur, k.stop_bit = w.end_bit, k.text_at = text, k.len = w.n;
            k.avail = static_cast<uint32_t>(std::min<uint64_t>(gz::kWindow, Z.front + member_len));
            k.piece0 = pieces;
            k.last_mul = gz::crc_x_pow8(w.n % gz::kPiece ? w.n % gz::kPiece : (w.n ? gz::kPiece : 0u));
            pieces += static_cast<uint32_t>((w.n + gz::kPiece - 1u) / gz::kPiece);
            Z.ready.push_back(k);
            text += w.n;
            member_len += w.n;
            cur = w.end_bit;
        }
        if (cur > stop)
            return fail(c, SLIMM_E_SPLIT, "gzip: the chain steps over the range's end, bit %llu: the block there ends at bit %llu",
                        static_cast<unsigned long long>(W.announced.gz_end_bit), static_cast<unsigned long long>(T.base * 8u + cur));
        if (w.status == gz::kRanOut) {
            if (last) {
                T.bit = cur;
                return ends_mid ? gz_short_of_end(c) : GZ_TRUNCATED();
            }
            T.waiting = true;
            break;
        }
        if (w.final) {
            final = true;
            break;
        }
        if (cur == stop) break;
        const size_t nx = static_cast<size_t>(std::lower_bound(starts.begin() + static_cast<long>(i) + 1, starts.end(), cur) - starts.begin());
        if (nx >= ns || starts[nx] != cur) break;   // (stopped behind kChunkTextSoft bytes of text: an exact start for the next round)
        i = nx;
    }
    // (the chunk starts the chain has passed that are no chunk of it: no blocks start there)
    size_t chained = 0;
    for (const gz::Chunk& k : Z.ready) chained += std::binary_search(starts.begin(), starts.end(), k.start_bit) ? 1u : 0u;
    stats[WindowPipeline::kGzDropped] += static_cast<uint64_t>(std::lower_bound(starts.begin(), starts.end(), cur) - starts.begin()) - chained;
    stats[WindowPipeline::kGzChunks] += Z.ready.size();
    T.bit = cur;
    if (final) Z.stage = Stage::Trailer;
    if (cur == stop && !final) Z.range_done = true;
    return SLIMM_OK;
}

// A round of the window pass: the chain's chunks decoded as in gz_emit, and their last 32 768 symbols propagated in 16 bits
// (k_gz_windows16) instead of resolved: no text, no CRC; slot 0 keeps the round's last window for the next round, and
// behind the last round for slimm_group_gzip_windows.  Memory: one round's
int gz_window_round(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    WindowPipeline::File::Gzip& Z = W.file.gz;
    WindowPipeline::Gzip& S = W.gz;
    hipStream_t st = c->stream;
    const uint32_t n = static_cast<uint32_t>(Z.ready.size());
    uint64_t text = 0;
    for (const gz::Chunk& k : Z.ready) text += k.len;
    if (S.chunks.cap < n) HIP_TRY(c, S.chunks.ensure_later(n + (n >> 2) + 64u, W.outgrown));
    if (S.sym.cap < text + 1u) HIP_TRY(c, S.sym.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    const uint64_t win_need = (static_cast<uint64_t>(n) + 1u) * gz::kWindow;
    if (S.win16.cap < win_need) {
        const uint64_t room = win_need + (win_need >> 2);
        if (Z.carried) HIP_TRY(c, S.win16.grow_keeping(room, 0, gz::kWindow, st, false, &W.outgrown));
        else
            HIP_TRY(c, S.win16.ensure_later(room, W.outgrown));
    }
    const bool identity = !Z.carried && W.announced.starts_mid;
    if (!Z.carried && !identity) HIP_TRY(c, hipMemsetAsync(S.win16.p, 0, gz::kWindow * sizeof(uint16_t), st));
    HIP_TRY(c, hipMemcpyAsync(S.chunks.p, Z.ready.data(), n * sizeof(gz::Chunk), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_decode, dim3(n), dim3(64), 0, st, S.comp.p, W.file.stream.pend.size(), S.chunks.p, n, S.sym.p);
    hipLaunchKernelGGL(k_gz_windows16, dim3(1), dim3(1024), 0, st, S.chunks.p, n, S.sym.p, S.win16.p, identity ? 1u : 0u);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(S.win16.p, S.win16.p + static_cast<uint64_t>(n) * gz::kWindow, gz::kWindow * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.chunks.p, n * sizeof(gz::Chunk), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    Z.carried = true;
    for (const gz::Chunk& k : Z.ready) {
        if (k.status != gz::kOk) return gz_bad_blocks(c, k.status);
        Z.len += k.len;
    }
    Z.text += text;
    push_trace_gz("window pass, round %llu: %u chunks, %.1f MB of text passed over", (unsigned long long)W.gz_stats[WindowPipeline::kGzRounds], n, text / 1e6);
    Z.ready.clear();
    return SLIMM_OK;
}

int gz_emit(slimm_ctx* c, uint8_t* dst, uint64_t, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline& W = c->win;
    WindowPipeline::File::Gzip& Z = W.file.gz;
    WindowPipeline::Gzip& S = W.gz;
    hipStream_t st = c->stream;
    uint64_t* stats = W.gz_stats;
    const uint32_t n = static_cast<uint32_t>(Z.ready.size());
    *n_out = 0;
    if (!n) return SLIMM_OK;
    if (Z.window_pass) return gz_window_round(c);
    uint64_t text = 0;
    for (const gz::Chunk& k : Z.ready) text += k.len;
    const uint32_t pieces = Z.ready.back().piece0 + static_cast<uint32_t>((Z.ready.back().len + gz::kPiece - 1u) / gz::kPiece);
    const uint64_t drop = W.file.stream.skip_of(text);
    if (S.chunks.cap < n) HIP_TRY(c, S.chunks.ensure_later(n + (n >> 2) + 64u, W.outgrown));
    if (S.sym.cap < text + 1u) HIP_TRY(c, S.sym.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    if (S.piece.cap < pieces + 1u) HIP_TRY(c, S.piece.ensure_later(pieces + (pieces >> 3) + 1u, W.outgrown));
    const uint64_t win_need = (static_cast<uint64_t>(n) + 1u) * gz::kWindow;
    if (S.win.cap < win_need) {   // (slot 0 -- the last 32 768 bytes of the text so far -- moves with it)
        const uint64_t room = win_need + (win_need >> 2);
        if (Z.carried) HIP_TRY(c, S.win.grow_keeping(room, 0, gz::kWindow, st, false, &W.outgrown));
        else
            HIP_TRY(c, S.win.ensure_later(room, W.outgrown));
    }
    if (!Z.carried) {
        // (a range that starts among a member's blocks: the bytes in front of it, as the window pass of its left neighbour left them)
        if (W.announced.gz_range && W.announced.starts_mid && W.gz_pass.has_front)
            HIP_TRY(c, hipMemcpyAsync(S.win.p, S.front.p, gz::kWindow, hipMemcpyDeviceToDevice, st));
        else
            HIP_TRY(c, hipMemsetAsync(S.win.p, 0, gz::kWindow, st));
    }
    HIP_TRY(c, hipMemcpyAsync(S.chunks.p, Z.ready.data(), n * sizeof(gz::Chunk), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_decode, dim3(n), dim3(64), 0, st, S.comp.p, W.file.stream.pend.size(), S.chunks.p, n, S.sym.p);
    hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(1024), 0, st, S.chunks.p, n, S.sym.p, S.win.p);
    if (pieces)
        hipLaunchKernelGGL(k_gz_resolve, dim3((pieces + 255u) / 256u), dim3(256), 0, st, S.chunks.p, n, pieces, S.sym.p, S.win.p, drop, dst, S.piece.p);
    hipLaunchKernelGGL(k_gz_fold, dim3((n + 63u) / 64u), dim3(64), 0, st, S.chunks.p, n, S.piece.p, gz::crc_x_pow8(gz::kPiece));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(S.win.p, S.win.p + static_cast<uint64_t>(n) * gz::kWindow, gz::kWindow, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.chunks.p, n * sizeof(gz::Chunk), hipMemcpyDeviceToHost, st));
    if (text > drop) HIP_TRY(c, hipMemcpyAsync(last_byte, dst + (text - drop) - 1u, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    Z.carried = true;
    for (const gz::Chunk& k : Z.ready) {
        // (a decode error here is one on the chain: the size pass took these blocks, so only a reach in front of the
        // member's start, which it cannot see, is expected)
        if (k.status != gz::kOk) return gz_bad_blocks(c, k.status);
        Z.crc = gz::crc_mul(Z.crc, gz::crc_x_pow8(k.len)) ^ k.crc;
        Z.len += k.len;
        stats[WindowPipeline::kGzStored] += k.kinds[0];
        stats[WindowPipeline::kGzFixed] += k.kinds[1];
        stats[WindowPipeline::kGzDynamic] += k.kinds[2];
        stats[WindowPipeline::kGzResolved] += k.markers;
    }
    stats[WindowPipeline::kGzText] += text;
    Z.text += text;
    *n_out = text - drop;
    push_trace_gz("round %llu: %u chunks -> %.1f MB of text", (unsigned long long)stats[WindowPipeline::kGzRounds], n, text / 1e6);
    Z.ready.clear();
    return SLIMM_OK;
}

void launch_gz_window_apply(hipStream_t st, const uint16_t* win16, const uint8_t* front, uint8_t* out) {
    hipLaunchKernelGGL(k_gz_window_apply, dim3(gz::kWindow / 256u), dim3(256), 0, st, win16, front, out);
}

void gz_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const uint64_t* s = c->win.gz_stats;
    fprintf(stderr, "[push gzip] %llu members, %llu chunks in %llu rounds, %llu candidates (%llu dropped); blocks: %llu stored, %llu fixed, "
                    "%llu dynamic; %llu bytes resolved from the chunk in front; %llu bytes of text\n",
            (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[8], (unsigned long long)s[2], (unsigned long long)s[3],
            (unsigned long long)s[4], (unsigned long long)s[5], (unsigned long long)s[6], (unsigned long long)s[7], (unsigned long long)s[9]);
}

// ---- a file split by byte range over a group's members: this codec's check in slimm_group_stitch_ranges (windows.h)
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
        ran[k] = F.active && F.closed && c->win.file.stream.codec == WindowPipeline::File::Codec::Gzip && F.gz.window_pass;
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
        if (c->win.file.stream.codec != WindowPipeline::File::Codec::Gzip || !A.gz_range) return fail(c, SLIMM_E_INVALID, "a range of a gzip file: slimm_set_gzip_range tells where it lies");
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

}  // namespace slimm
