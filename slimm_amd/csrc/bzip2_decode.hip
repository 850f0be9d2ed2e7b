// bzip2-compressed SAM decoded on the device (include/slimm_hip.h: slimm_push_bzip2_sam_bytes; the block format:
// bzip2_block.h).  The host cannot know where a block ends, nor how much text it holds, without decoding it, so a window of
// compressed bytes goes through stages:
//   k_bz2_find    every bit offset of the bytes: the 48-bit block magic there?  Candidates -- a magic may also occur by
//                 chance inside compressed data (2^-48 per bit), so none is trusted
//   k_bz2_decode  a WAVE per candidate of a batch (lane 0; the block's tables in LDS): Huffman, selectors, MTF, RUNA/RUNB
//                 -> the block's BWT string, its byte histogram, where it ended (or that the bytes ran out)
//   (host)        the chain: from the first block, known real, each block's end to the next magic, end-of-stream markers
//                 (combined CRC, padding, a next "BZh" stream) checked on the host's copy of the bytes; candidates
//                 inside real blocks are dropped; a block that ran out of bytes waits, with its bytes, for the next push
//   k_bz2_unbwt   a workgroup per block: the inverse BWT's links (a counting sort), then the walk from origPtr cut at
//                 rulers (every kRuler-th position): each thread walks from a ruler to the next, the rulers of the cycle
//                 through origPtr are put in order, each walk is repeated writing its bytes in place (a text that repeats
//                 itself has several cycles: the one through origPtr is repeated, as bzip2's n-step walk does); then the
//                 RLE1 text's length
//   k_bz2_emit    a wave per block: RLE1 undone into the window buffer behind the blocks in front of it (the lengths'
//                 prefix sum), contiguous as the SAM decoder wants it, the block's CRC checked
// The window then goes to the SAM finder and decoder as any text window does (windows.hip).
#include "context.h"

namespace slimm {
namespace {

constexpr uint32_t kRuler = 256;   // positions between two rulers of the inverse BWT's walk
constexpr uint32_t kMaxRulers = bz2::kMaxBlock / kRuler + 2;
constexpr uint64_t kBz2Tail = 16;  // zeroed bytes behind the compressed bytes on the device

__global__ __launch_bounds__(256) void k_bz2_find(const uint8_t* __restrict__ b, uint64_t n_bytes, uint64_t bit_lo, uint64_t bit_hi,
                                                   unsigned long long* __restrict__ cand, uint32_t* __restrict__ count, uint32_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = (bit_lo >> 3) + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_bytes; i += stride) {
        uint64_t v = 0;   // bytes i .. i + 7, the first one highest (the buffer has kBz2Tail zeroed bytes behind n_bytes)
        for (uint32_t k = 0; k < 8; ++k) v = (v << 8) | b[i + k];
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t bit = i * 8u + k;
            if (bit < bit_lo || bit + 48u > bit_hi) continue;
            if (((v >> (16u - k)) & 0xffffffffffffull) == bz2::kBlockMagic) {
                const uint32_t at = atomicAdd(count, 1u);
                if (at < cap) cand[at] = bit;
            }
        }
    }
}

// A range that starts inside the file (a file split by byte range): the first end-of-stream magic whose first bit lies in
// [bit_lo, bit_hi) -- the range's first element may be a marker, which no block decode vouches for; the stitch does
// (split_bz2_chains, below).  *first: ~0 before, the smallest such bit after
__global__ __launch_bounds__(256) void k_bz2_first_eos(const uint8_t* __restrict__ b, uint64_t n_bytes, uint64_t bit_lo, uint64_t bit_hi,
                                                        unsigned long long* __restrict__ first) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t hi_byte = (bit_hi + 7u) >> 3, stop = hi_byte < n_bytes ? hi_byte : n_bytes;
    for (uint64_t i = (bit_lo >> 3) + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < stop; i += stride) {
        uint64_t v = 0;   // bytes i .. i + 7, the first one highest (the buffer has kBz2Tail zeroed bytes behind n_bytes)
        for (uint32_t k = 0; k < 8; ++k) v = (v << 8) | b[i + k];
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t bit = i * 8u + k;
            if (bit < bit_lo || bit >= bit_hi || bit + 48u > n_bytes * 8u) continue;
            if (((v >> (16u - k)) & 0xffffffffffffull) == bz2::kEosMagic) atomicMin(first, static_cast<unsigned long long>(bit));
        }
    }
}

__global__ __launch_bounds__(64) void k_bz2_decode(const uint8_t* __restrict__ b, uint64_t end_bit, const unsigned long long* __restrict__ cand,
                                                    uint8_t* __restrict__ ll, uint32_t* __restrict__ hist, bz2::BlockInfo* __restrict__ info) {
    __shared__ bz2::Tables t;
    if (threadIdx.x != 0) return;
    const uint32_t s = blockIdx.x;
    bz2::BlockInfo r;
    bz2::decode_block(b, cand[s], end_bit, bz2::kMaxBlock, t, ll + static_cast<uint64_t>(s) * bz2::kMaxBlock, hist + s * 256u, r);
    info[s] = r;
}

// text_len[k] = the RLE1 text's bytes of the block in slot slots[k]; kLenBadLinks: its links are no permutation (never for
// links made by link_block: a guard against an out-of-range walk); kLenBadRun: it ends in four equal bytes without a count byte
__global__ __launch_bounds__(256) void k_bz2_unbwt(const uint32_t* __restrict__ slots, const bz2::BlockInfo* __restrict__ info,
                                                    uint8_t* __restrict__ ll_all, uint32_t* __restrict__ link_all, const uint32_t* __restrict__ hist,
                                                    uint32_t* __restrict__ text_len) {
    __shared__ uint32_t r_len[kMaxRulers], r_next[kMaxRulers], r_off[kMaxRulers];
    __shared__ uint32_t cf[256];
    __shared__ uint32_t bad, period;
    const uint32_t s = slots[blockIdx.x];
    const uint32_t n = info[s].n, orig = info[s].orig_ptr;
    uint8_t* ll = ll_all + static_cast<uint64_t>(s) * bz2::kMaxBlock;
    uint32_t* link = link_all + static_cast<uint64_t>(s) * bz2::kMaxBlock;
    if (threadIdx.x == 0) {
        bz2::link_block(ll, n, hist + s * 256u, link, cf);
        bad = 0;
    }
    __syncthreads();
    // the rulers: positions r * kRuler, and origPtr (index nr) unless it is one of them
    const uint32_t nr = (n + kRuler - 1u) / kRuler, total = nr + (orig % kRuler ? 1u : 0u);
    auto ruler_of = [&](uint32_t p) -> uint32_t { return p % kRuler == 0 ? p / kRuler : (p == orig ? nr : ~0u); };
    auto ruler_pos = [&](uint32_t r) -> uint32_t { return r < nr ? r * kRuler : orig; };
    for (uint32_t r = threadIdx.x; r < total; r += blockDim.x) {
        uint32_t p = ruler_pos(r), len = 0, nx;
        do {
            p = link[p] & bz2::kLinkMask;
            ++len;
            nx = p < n ? ruler_of(p) : ~1u;
        } while (nx == ~0u && len <= n);
        r_len[r] = len;
        r_next[r] = nx;
        r_off[r] = ~0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // the rulers of the cycle through origPtr in the walk's order: where each one's stretch of the text starts, until
        // the cycle closes after `period` positions (n, unless the text repeats itself)
        const uint32_t first = ruler_of(orig);
        uint32_t r = first, off = 0;
        do {
            if (r >= total || r_off[r] != ~0u || r_len[r] > n - off) {
                bad = 1;
                break;
            }
            r_off[r] = off;
            off += r_len[r];
            r = r_next[r];
        } while (r != first);
        period = off;
        if (off == 0) bad = 1;
    }
    __syncthreads();
    if (bad) {
        if (threadIdx.x == 0) text_len[blockIdx.x] = bz2::kLenBadLinks;
        return;
    }
    for (uint32_t r = threadIdx.x; r < total; r += blockDim.x) {
        uint32_t p = ruler_pos(r), o = r_off[r];
        if (o == ~0u) continue;   // (a ruler of another cycle)
        const uint32_t e = o + r_len[r];
        for (; o < e; ++o) {
            const uint32_t u = link[p];
            ll[o] = static_cast<uint8_t>(u >> 24);
            p = u & bz2::kLinkMask;
        }
    }
    __syncthreads();
    // n steps round a cycle of `period` positions: the stretch again and again (reads below `period`, writes above it)
    for (uint32_t k = period + threadIdx.x; k < n; k += blockDim.x) ll[k] = ll[k % period];
    __syncthreads();
    if (threadIdx.x == 0) {
        bz2::Rle1 st;
        uint32_t len = 0, byte;
        for (uint32_t k = 0; k < n; ++k) len += st.step(ll[k], byte);
        text_len[blockIdx.x] = st.count_missing() ? bz2::kLenBadRun : len;
    }
}

// the RLE1 text of block k (slot slots[k]) into dst: its byte j at dst[at[2k] + j] for j >= at[2k + 1] (bytes in front are
// skipped: the header); crc_ok[k] = its CRC matches
__global__ __launch_bounds__(64) void k_bz2_emit(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ ll_all,
                                                  const bz2::BlockInfo* __restrict__ info, const int64_t* __restrict__ at, uint8_t* __restrict__ dst,
                                                  uint32_t* __restrict__ crc_ok) {
    __shared__ uint32_t tab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : (c << 1);
        tab[i] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t s = slots[blockIdx.x], n = info[s].n;
    const uint8_t* ll = ll_all + static_cast<uint64_t>(s) * bz2::kMaxBlock;
    const int64_t base = at[2u * blockIdx.x], drop = at[2u * blockIdx.x + 1u];
    bz2::Rle1 st;
    uint32_t crc = 0xffffffffu, byte;
    int64_t j = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t copies = st.step(ll[k], byte);
        for (uint32_t c = 0; c < copies; ++c, ++j) {
            crc = bz2::crc_byte(tab, crc, byte);
            if (j >= drop) dst[base + j] = static_cast<uint8_t>(byte);
        }
    }
    crc_ok[blockIdx.x] = ~crc == info[s].crc && !st.count_missing() ? 1u : 0u;   // (k_bz2_unbwt refused a missing count byte)
}

void push_trace_bz2(const char* fmt, ...) {   // "[push bzip2] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("bzip2", fmt, ap);
    va_end(ap);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

#define BZ2_FAIL(fmt, ...) fail(c, SLIMM_E_INVALID, "bzip2-compressed input is not supported unless it decodes: " fmt, __VA_ARGS__)
// a range that ends inside the file ran out of bytes: the slack behind it (bz2::kSplitSlack) did not finish its last block
#define BZ2_SLACK_FAIL(what, at) \
    fail(c, SLIMM_E_SPLIT, "bzip2: %s at byte %llu is not finished by the %llu bytes read behind the range", what, at, (unsigned long long)bz2::kSplitSlack)

// the block magics of pend from T.bit on, in order: the bytes go to the device first
int bz2_find(slimm_ctx* c) {
    WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    WindowPipeline::File::Stream& T = c->win.file.stream;
    WindowPipeline::Bzip2& S = c->win.bz2;
    hipStream_t st = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = T.pend.size();
    SLIMM_TRY(stream_upload(c, S.comp, kBz2Tail));
    HIP_TRY(c, S.count.ensure(4));
    uint32_t got = 0;
    // (more magics than room: blocks of a few bytes each, pbzip2 on a tiny input)
    SLIMM_TRY(stream_candidates(c, S.d_cand, S.count, static_cast<uint32_t>(std::min<uint64_t>(n / 64u + 256u, 1u << 26)), [&](uint32_t cap) {
        const uint64_t span = n > (T.bit >> 3) ? n - (T.bit >> 3) : 0;
        const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>((span + 255u) / 256u, 4096u)));
        if (span) hipLaunchKernelGGL(k_bz2_find, dim3(grid), dim3(256), 0, st, S.comp.p, n, T.bit, n * 8u, S.d_cand.p, S.count.p, cap);
    }, &got));
    T.cand.resize(got);
    if (got) HIP_TRY(c, hipMemcpy(T.cand.data(), S.d_cand.p, got * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::sort(T.cand.begin(), T.cand.end());
    long every = 0;
    if (forced("bzip2_false_magics", &every)) {
        // (tests: candidates that are no blocks -- a few bits into every real one, and every `every` bits, 4096 by default
        // -- must be decoded and dropped without changing anything)
        const uint64_t step = every > 1 ? static_cast<uint64_t>(every) : 4096u;
        std::vector<uint64_t> extra;
        for (uint64_t b : T.cand) extra.push_back(b + 13u);
        for (uint64_t b = T.bit + 5u; b + 48u <= n * 8u; b += step) extra.push_back(b);
        T.cand.insert(T.cand.end(), extra.begin(), extra.end());
        std::sort(T.cand.begin(), T.cand.end());
        T.cand.erase(std::unique(T.cand.begin(), T.cand.end()), T.cand.end());
    }
    const WindowPipeline::Announced& A = c->win.announced;
    if (A.has_range && A.ends_mid) {   // (blocks that start at or behind the range's end are the next member's)
        const uint64_t lim = A.range_end > T.base ? (A.range_end - T.base) * 8u : 0u;
        T.cand.erase(std::lower_bound(T.cand.begin(), T.cand.end(), lim), T.cand.end());
    }
    Z.next_cand = 0;
    T.found = true;
    Z.ms_find += ms_since(t0);
    return SLIMM_OK;
}

// the first end-of-stream magic of the bytes on the device whose first bit lies in [lo, hi): *bit (~0: none)
int bz2_first_eos(slimm_ctx* c, uint64_t lo, uint64_t hi, uint64_t* bit) {
    WindowPipeline::Bzip2& S = c->win.bz2;
    hipStream_t st = c->stream;
    const uint64_t n = c->win.file.stream.pend.size();
    unsigned long long* d_first = reinterpret_cast<unsigned long long*>(S.count.p + 2);   // (count holds four words)
    unsigned long long got = ~0ull;
    *bit = ~0ull;
    if (lo >= hi || lo + 48u > n * 8u) return SLIMM_OK;
    HIP_TRY(c, hipMemsetAsync(d_first, 0xff, sizeof(got), st));
    const uint64_t span = std::min<uint64_t>(n, (hi + 7u) >> 3) - (lo >> 3);
    const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>((span + 255u) / 256u, 4096u)));
    hipLaunchKernelGGL(k_bz2_first_eos, dim3(grid), dim3(256), 0, st, S.comp.p, n, lo, hi, d_first);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&got, d_first, sizeof(got), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *bit = got;
    return SLIMM_OK;
}

// the decode scratch for `slots` blocks at a time, once per file
int bz2_reserve(slimm_ctx* c) {
    WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    WindowPipeline::Bzip2& S = c->win.bz2;
    if (Z.slots) return SLIMM_OK;
    // (a batch of blocks: as many as the file has, about -- a 900 k block compresses SAM text to 60 - 250 kB --, 16 to 256)
    const uint64_t hint = c->win.announced.size_hint;
    Z.slots = hint ? static_cast<uint32_t>(std::min<uint64_t>(256u, std::max<uint64_t>(16u, hint / 65536u + 2u))) : 64u;
    HIP_TRY(c, S.ll.ensure(static_cast<size_t>(Z.slots) * bz2::kMaxBlock));
    HIP_TRY(c, S.link.ensure(static_cast<size_t>(Z.slots) * bz2::kMaxBlock));
    HIP_TRY(c, S.hist.ensure(static_cast<size_t>(Z.slots) * 256u));
    HIP_TRY(c, S.info.ensure(Z.slots));
    HIP_TRY(c, S.text_len.ensure(2u * Z.slots));
    HIP_TRY(c, S.out_at.ensure(2u * Z.slots));
    if (hint && S.comp.cap < hint + kBz2Tail) {
        const uint64_t comp = std::min<uint64_t>(hint, 448ull << 20) + kBz2Tail;   // (a window: the pushes since the last batch)
        HIP_TRY(c, S.comp.ensure(comp));
        HIP_TRY(c, S.d_cand.ensure(comp / 64u + 256u));
    }
    push_trace_bz2("%u blocks a batch: %.0f MB of decode scratch", Z.slots, S.held() / 1e6);
    return SLIMM_OK;
}

}  // namespace

int bz2_decode_batch(slimm_ctx* c, bool last) {
    WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    WindowPipeline::File::Stream& T = c->win.file.stream;
    WindowPipeline::Bzip2& S = c->win.bz2;
    hipStream_t st = c->stream;
    WindowPipeline::File::Bzip2::Chain& K = Z.chain;
    const WindowPipeline::Announced& A = c->win.announced;
    const bool starts_mid = A.has_range && A.starts_mid, ends_mid = A.has_range && A.ends_mid;
    Z.ready.clear();
    Z.ready_pos = 0;
    if (K.ended) return SLIMM_OK;              // (a range that ends inside the file: what is left of the slack is dropped)
    if (T.waiting && !last) return SLIMM_OK;   // (no byte has come since the chain stopped for want of them)
    SLIMM_TRY(bz2_reserve(c));
    if (!T.found) {
        SLIMM_TRY(bz2_find(c));
    }
    const uint64_t end_bit = T.pend.size() * 8u;
    auto at = [&](uint64_t bit) { return static_cast<unsigned long long>(T.base + (bit >> 3)); };
    std::vector<bz2::BlockInfo> hinfo;
    size_t batch0 = 0, nb = 0;   // the batch: candidates [batch0, batch0 + nb) in slots 0 .. nb - 1
    std::vector<uint32_t> slots;
    std::vector<uint32_t> crcs;
    std::vector<uint64_t> ats;
    auto abs_bit = [&](uint64_t bit) { return T.base * 8u + bit; };
    // the batch of candidates from `from` on decoded into slots 0 .. nb - 1
    auto decode_from = [&](size_t from) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        batch0 = from;
        nb = std::min<size_t>(Z.slots, T.cand.size() - batch0);
        HIP_TRY(c, hipMemcpyAsync(S.d_cand.p, T.cand.data() + batch0, nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bz2_decode, dim3(static_cast<uint32_t>(nb)), dim3(64), 0, st, S.comp.p, end_bit, S.d_cand.p, S.ll.p, S.hist.p,
                           S.info.p);
        HIP_TRY(c, hipGetLastError());
        hinfo.resize(nb);
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), S.info.p, nb * sizeof(bz2::BlockInfo), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        Z.ms_decode += ms_since(t0);
        ++Z.batches;
        return SLIMM_OK;
    };
    if (starts_mid && !K.started) {
        // A range that starts inside the file: its chain starts at its first element -- the first candidate that decodes
        // (those in front of it are false magics), or an end-of-stream marker in front of that one -- inside a stream of
        // unknown level.  Nothing vouches for that start but the member on the left, whose chain must end there
        // (SLIMM_FORCE bzip2_split_wrong_first: the first element is passed over, the chain starts at the one behind it)
        const uint64_t range_end_bit = ends_mid ? (A.range_end > T.base ? (A.range_end - T.base) * 8u : 0u) : end_bit;
        uint64_t lo = T.bit, first = ~0ull;
        size_t i = Z.next_cand;
        for (int pass = forced("bzip2_split_wrong_first") ? 2 : 1; pass > 0; --pass) {
            bool have_block = false;
            for (; i < T.cand.size(); ++i) {
                if (T.cand[i] < lo) continue;
                if (i < batch0 || i >= batch0 + nb) SLIMM_TRY(decode_from(i));
                const uint32_t status = hinfo[i - batch0].status;
                if (status == bz2::kRanOut && !last) break;   // (its bytes go on with the next push: no verdict yet)
                if (status != bz2::kOk) continue;
                have_block = true;
                break;
            }
            if (!have_block && !last) {
                T.waiting = true;
                return SLIMM_OK;
            }
            SLIMM_TRY(bz2_first_eos(c, lo, std::min(have_block ? T.cand[i] : end_bit, range_end_bit), &first));
            if (have_block) first = std::min<uint64_t>(first, T.cand[i]);
            if (first == ~0ull) break;
            lo = first + 1u;   // (forced: the element behind the first one)
        }
        const size_t next = static_cast<size_t>(std::lower_bound(T.cand.begin(), T.cand.end(), first) - T.cand.begin());
        Z.false_magics += next - Z.next_cand;
        Z.next_cand = next;
        K.started = true;
        if (first == ~0ull) {   // (no block or marker starts in the range: an empty member)
            K.ended = true;
            K.end_bit = abs_bit(T.bit);
            return SLIMM_OK;
        }
        T.bit = first;
        Z.in_stream = K.first_stream = K.any = true;
        Z.level = 9;
        Z.combined = 0;
        Z.streams = 1;
        K.first_bit = abs_bit(first);
        push_trace_bz2("the range's chain starts at bit %llu (byte %llu)", (unsigned long long)K.first_bit, at(first));
    }
    for (;;) {
        if (!Z.in_stream) {   // a stream header, at a byte
            const uint64_t byte = T.bit >> 3;
            const uint64_t avail = T.pend.size() - byte;
            const uint8_t* h = T.pend.data() + byte;
            if (avail == 0) {
                if (last && Z.streams == 0) return BZ2_FAIL("truncated at byte %llu", at(T.bit));
                T.waiting = true;
                K.at_file_end = last;
                break;
            }
            if (avail < 4 && !last && memcmp(h, "BZh", avail) == 0) {
                T.waiting = true;
                break;
            }
            if (avail < 4 || memcmp(h, "BZh", 3) != 0 || h[3] < '1' || h[3] > '9') {
                if (avail < 4 && memcmp(h, "BZh", avail) == 0) return BZ2_FAIL("truncated stream header at byte %llu", at(T.bit));
                if (Z.streams) return BZ2_FAIL("bytes after the last end-of-stream marker, at byte %llu", at(T.bit));
                return BZ2_FAIL("not a bzip2 stream%s", "");
            }
            Z.level = static_cast<uint32_t>(h[3] - '0');
            Z.combined = 0;
            Z.in_stream = true;
            ++Z.streams;
            T.bit += 32;
        }
        // (a range that ends inside the file: the element -- a block, or a marker with the stream header behind it -- that
        // starts at or behind the range's end is the next member's)
        if (ends_mid && abs_bit(T.bit) >= A.range_end * 8u) {
            K.ended = true;
            break;
        }
        bz2::Bits br(T.pend.data(), T.bit, end_bit);
        uint64_t magic;
        if (!br.peek48(magic)) {
            if (last && ends_mid) return BZ2_SLACK_FAIL("what starts", at(T.bit));
            if (last) return BZ2_FAIL("truncated at byte %llu", at(T.bit));
            T.waiting = true;
            break;
        }
        if (magic == bz2::kEosMagic) {
            uint32_t v, hi, lo;
            if (!br.get(24, v) || !br.get(24, v) || !br.get(16, hi) || !br.get(16, lo)) {
                if (last && ends_mid) return BZ2_SLACK_FAIL("the end-of-stream marker", at(T.bit));
                if (last) return BZ2_FAIL("truncated end-of-stream marker at byte %llu", at(T.bit));
                T.waiting = true;
                break;
            }
            if (K.first_stream) {   // (the stream the range started in: the stitch knows what came before)
                K.first_stream = false;
                K.has_eos = true;
                K.first_combined = Z.combined;
                K.eos_crc = (hi << 16) | lo;
                K.eos_at = at(T.bit);
            } else if (((hi << 16) | lo) != Z.combined) {
                if (!slots.empty()) break;   // (the blocks in front go first: a block CRC that does not match is named as such)
                return BZ2_FAIL("end-of-stream marker at byte %llu: combined CRC mismatch", at(T.bit));
            }
            T.bit = (br.pos() + 7u) & ~7ull;
            Z.in_stream = false;
            K.any = true;
            continue;
        }
        if (magic != bz2::kBlockMagic) return BZ2_FAIL("at byte %llu: %s", at(T.bit), bz2::status_text(bz2::kNoBlock));
        // a block: decoded in the batch at hand, or first in a new batch (once the blocks of this one are through)
        while (Z.next_cand < T.cand.size() && T.cand[Z.next_cand] < T.bit) {   // (magics inside the blocks in front: no blocks)
            ++Z.next_cand;
            ++Z.false_magics;
        }
        if (Z.next_cand >= T.cand.size() || T.cand[Z.next_cand] != T.bit)
            return fail(c, SLIMM_E_INVALID, "bzip2: the block magic at byte %llu was not found by the device's scan", at(T.bit));
        if (Z.next_cand < batch0 || Z.next_cand >= batch0 + nb) {
            if (!slots.empty()) break;
            SLIMM_TRY(decode_from(Z.next_cand));
        }
        const uint32_t s = static_cast<uint32_t>(Z.next_cand - batch0);
        const bz2::BlockInfo& r = hinfo[s];
        if (r.status == bz2::kRanOut) {   // (the block's bytes go on with the next push)
            if (last && ends_mid) return BZ2_SLACK_FAIL("the block", at(T.bit));
            if (last) return BZ2_FAIL("block at byte %llu: truncated", at(T.bit));
            T.waiting = true;
            break;
        }
        if (r.status != bz2::kOk) return BZ2_FAIL("block at byte %llu: %s", at(T.bit), bz2::status_text(r.status));
        if (r.n > Z.level * 100000u) return BZ2_FAIL("block at byte %llu: %s", at(T.bit), bz2::status_text(bz2::kTooLong));
        if (K.first_stream) {   // (level unknown: the stitch holds the largest block against the left chain's level)
            ++K.first_blocks;
            if (r.n > K.first_max_n) K.first_max_n = r.n, K.first_max_at = at(T.bit);
        }
        K.any = true;
        slots.push_back(s);
        crcs.push_back(r.crc);
        ats.push_back(at(T.bit));
        Z.combined = ((Z.combined << 1) | (Z.combined >> 31)) ^ r.crc;
        T.bit = r.end_bit;
        ++Z.next_cand;
    }
    K.end_bit = abs_bit(T.bit);
    if (slots.empty()) return SLIMM_OK;
    // the blocks of the chain: inverse BWT, text lengths
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t k = static_cast<uint32_t>(slots.size());
    HIP_TRY(c, hipMemcpyAsync(S.text_len.p + Z.slots, slots.data(), k * 4u, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bz2_unbwt, dim3(k), dim3(256), 0, st, S.text_len.p + Z.slots, S.info.p, S.ll.p, S.link.p, S.hist.p, S.text_len.p);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> len(k);
    HIP_TRY(c, hipMemcpyAsync(len.data(), S.text_len.p, k * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    Z.ms_bwt += ms_since(t0);
    for (uint32_t i = 0; i < k; ++i) {
        if (len[i] == bz2::kLenBadLinks || len[i] == bz2::kLenBadRun)
            return BZ2_FAIL("block at byte %llu: %s", static_cast<unsigned long long>(ats[i]),
                            bz2::status_text(len[i] == bz2::kLenBadRun ? bz2::kBadRun : bz2::kBadLinks));
        WindowPipeline::File::Bzip2::Ready b;
        b.slot = slots[i];
        b.crc = crcs[i];
        b.len = len[i];
        b.drop = T.skip_of(b.len);
        b.at = ats[i];
        b.unchecked = starts_mid && Z.blocks == 0 && i == 0;
        Z.ready.push_back(b);
    }
    Z.blocks += k;
    return SLIMM_OK;
}

void bz2_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    fprintf(stderr, "[push bzip2] %llu streams, %llu blocks in %llu batches, %llu false magics; find %.1f ms, decode %.1f ms, "
                    "inverse BWT %.1f ms, text %.1f ms\n", (unsigned long long)Z.streams, (unsigned long long)Z.blocks,
            (unsigned long long)Z.batches, (unsigned long long)Z.false_magics, Z.ms_find, Z.ms_decode, Z.ms_bwt, Z.ms_emit);
}

namespace {
// the text bytes of the next ready blocks that fit in `cap` (at least one block)
uint64_t bz2_window_bytes(const slimm_ctx* c, uint64_t cap, size_t* n_blocks) {
    const WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    uint64_t n = 0;
    size_t i = Z.ready_pos;
    for (; i < Z.ready.size(); ++i) {
        const uint64_t m = Z.ready[i].len - Z.ready[i].drop;
        if (i > Z.ready_pos && n + m > cap) break;
        n += m;
    }
    *n_blocks = i - Z.ready_pos;
    return n;
}
}  // namespace

bool bz2_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n) {
    size_t n_blocks = 0;
    *n = bz2_window_bytes(c, cap, &n_blocks);
    return n_blocks != 0;
}

int bz2_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline::File::Bzip2& Z = c->win.file.bz2;
    size_t n_blocks = 0;
    *n_out = bz2_window_bytes(c, cap, &n_blocks);
    WindowPipeline::Bzip2& S = c->win.bz2;
    hipStream_t st = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> slots(n_blocks);
    std::vector<int64_t> at(2 * n_blocks);
    int64_t off = 0;
    for (size_t i = 0; i < n_blocks; ++i) {
        const auto& b = Z.ready[Z.ready_pos + i];
        slots[i] = b.slot;
        at[2 * i] = off - static_cast<int64_t>(b.drop);
        at[2 * i + 1] = static_cast<int64_t>(b.drop);
        off += static_cast<int64_t>(b.len - b.drop);
    }
    const uint32_t k = static_cast<uint32_t>(n_blocks);
    HIP_TRY(c, hipMemcpyAsync(S.text_len.p + Z.slots, slots.data(), k * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(S.out_at.p, at.data(), at.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bz2_emit, dim3(k), dim3(64), 0, st, S.text_len.p + Z.slots, S.ll.p, S.info.p, S.out_at.p, dst, S.text_len.p);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> ok(k);
    HIP_TRY(c, hipMemcpyAsync(ok.data(), S.text_len.p, k * 4u, hipMemcpyDeviceToHost, st));
    if (off) HIP_TRY(c, hipMemcpyAsync(last_byte, dst + off - 1, 1, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    Z.ms_emit += ms_since(t0);
    for (uint32_t i = 0; i < k; ++i) {
        if (ok[i]) continue;
        const auto& b = Z.ready[Z.ready_pos + i];
        // (nothing but this CRC says that a range's first block is one: no verdict on the file)
        if (b.unchecked)
            return fail(c, SLIMM_E_SPLIT, "bzip2: the first block of a range that starts inside the file, at byte %llu: %s",
                        static_cast<unsigned long long>(b.at), bz2::status_text(bz2::kBadCrc));
        return BZ2_FAIL("block at byte %llu: %s", static_cast<unsigned long long>(b.at), bz2::status_text(bz2::kBadCrc));
    }
    Z.ready_pos += n_blocks;
    return SLIMM_OK;
}

// ---- a file split by byte range over a group's members: this codec's check in slimm_group_stitch_ranges (windows.h)
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

}  // namespace slimm
