// The copies of a round's text resolved: what the LZ codecs whose sequences are known before any text exists (zstd_decode.hip,
// lz4_decode.hip) share behind their expand kernels (windows.h: resolve_copies).  text: [history H | the round's n_text];
// src[i]: the position in it that byte H + i is a copy of (itself: a literal).  No workgroup waits for another: ordering
// comes from kernel boundaries only.
#include "context.h"

namespace slimm {
namespace {

__global__ __launch_bounds__(256) void k_zs_double(uint32_t* src, uint64_t H, uint64_t n_text, unsigned long long* __restrict__ count) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    bool changed = false;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_text; i += stride) {
        const uint32_t s = src[i];
        if (s < H || s == H + i) continue;   // (a byte of the history, or a literal: the chain's end)
        // (another thread may move src[s - H] on meanwhile: whatever is read there is a byte further up the same chain)
        const uint32_t t = src[s - H];
        if (t != s) {
            src[i] = t;
            changed = true;
        }
    }
    if (changed) count[0] = 1ull;
}

__global__ __launch_bounds__(256) void k_zs_gather(const uint32_t* __restrict__ src, uint8_t* __restrict__ text, uint64_t H, uint64_t n_text) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_text; i += stride) {
        const uint32_t s = src[i];
        if (s != H + i) text[H + i] = text[s];   // (s: a byte of the history or a literal; no match byte is read here)
    }
}

}  // namespace

uint32_t copy_grid_for(uint64_t n) { return static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>((n + 255u) / 256u, 16384u))); }

int resolve_copies(slimm_ctx* c, const char* codec, uint32_t* src, uint8_t* text, uint64_t H, uint64_t n_text, unsigned long long* count,
                   unsigned long long got[5], uint32_t* passes) {
    hipStream_t st = c->stream;
    // every pass halves what is left of the longest chain, and one more finds nothing to do
    uint32_t most = 1;
    while ((1ull << (most - 1u)) < n_text + H) ++most;
    for (;;) {
        hipLaunchKernelGGL(k_zs_double, dim3(copy_grid_for(n_text)), dim3(256), 0, st, src, H, n_text, count);
        HIP_TRY(c, hipGetLastError());
        ++*passes;
        HIP_TRY(c, hipMemcpyAsync(got, count, 5u * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemsetAsync(count, 0, sizeof(unsigned long long), st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (got[1]) return SLIMM_OK;
        if (!got[0]) break;
        if (*passes >= most) return fail(c, SLIMM_E_INVALID, "internal error: %s: the copies of a round did not resolve in %u passes", codec, most);
    }
    hipLaunchKernelGGL(k_zs_gather, dim3(copy_grid_for(n_text)), dim3(256), 0, st, src, text, H, n_text);
    HIP_TRY(c, hipGetLastError());
    return SLIMM_OK;
}

}  // namespace slimm
