// Internal to the library: the context behind the C ABI (include/slimm_hip.h) and what its translation units share --
// context.hip (create / reset, phases A and B, the getters), records.hip (decoded records in), windows.hip (a file's bytes in
// windows -- BAM records, BGZF blocks of them, SAM text, BGZF blocks of it, bzip2 SAM -- inflated and decoded on the device;
// its state: windows.h).
#pragma once
#include <cerrno>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/slimm_hip.h"
#include "host_profile.hpp"
#include "force.h"
#include "bzip2_block.h"
#include "deflate_stream.h"
#include "zstd_walk.h"
#include "xz_walk.h"
#include "lz4_walk.h"
#include "lzip_walk.h"
#include "kernels.h"
#include "read_identity.h"

namespace slimm {



extern thread_local std::string g_create_error;

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    // the same without hipFree (which waits for every kernel in flight on the device): what the buffer was goes to `old`,
    // whose owner frees it when the device has nothing to do anyway
    hipError_t ensure_later(size_t n, std::vector<void*>& old) {
        return n <= cap ? hipSuccess : grow_keeping(n, 0, 0, nullptr, false, &old);
    }
    // Grows to n elements keeping elements [from, from + count) where they are: copied on `st`, and waited for by the host
    // when `sync`.  What the buffer was goes to `old` (no hipFree now, as above); without one it is freed here
    hipError_t grow_keeping(size_t n, size_t from, size_t count, hipStream_t st, bool sync, std::vector<void*>* old) {
        DevBuf<T> nb;
        hipError_t e = nb.ensure(n);
        if (e == hipSuccess && count) e = hipMemcpyAsync(nb.p + from, p + from, count * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && sync) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        std::swap(p, nb.p);
        std::swap(cap, nb.cap);
        if (old && nb.p) {
            old->push_back(nb.p);
            nb.p = nullptr;
            nb.cap = 0;
        }
        return hipSuccess;
    }
};

template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    ~PinBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) cap = n;
        return e;
    }
};

enum KernelId {
    K_MEMSET = 0, K_GROUP_COUNT, K_GROUP_SCAN, K_GROUP_SCATTER, K_GROUP_FINISH, K_FRONT, K_HIST, K_REF_STATS, K_FILTER,
    K_REF_STATS2, K_TILE_COUNT, K_TILE_SCAN, K_TILE_SCATTER, K_TILE_HIST, K_TILE_COUNT2, K_TILE_SCAN2, K_TILE_SCATTER2,
    K_TILE_HIST2, K_PACK, K_PACK2, K_COUNT
};
extern const char* kKernelNames[K_COUNT];

constexpr uint32_t kTailWords = 64;

}  // namespace slimm

#include "windows.h"
#include "tile_bucketing.h"

using namespace slimm;   // (library-internal header)

struct slimm_ctx {
    std::unique_ptr<HostProfile> host;
    std::string err;
    int device = -1;  // -1: host-only context
    int order = SLIMM_ORDER_GROUPED;
    hipStream_t stream = nullptr;
    // streamed ingest (slimm_push_records_async): host -> device copies on a stream of their own, ordered before phase A
    // by an event (never by the host); two page-locked staging sets for callers that produce records piecemeal
    // Streams and HARDWARE QUEUES.  A process has few hardware queues per device (four of each priority class unless
    // GPU_MAX_HW_QUEUES says otherwise); the runtime deals streams to them as they are made, and streams that share one wait
    // for each other.  Which of the window pipeline's streams shared decided whether `slimm DB 100M.bam` spent 110-210 or
    // 320-360 ms in slimm_push_bgzf_blocks (every odd window's inflate 18 ms late), and differently for one context and for a
    // group's two members on one device (profiles/round6/11_*).  So the streams are told apart by PRIORITY CLASS, which the
    // runtime keeps in separate queue pools: the copy stream high (its work is the DMA engine's; what it needs is to be
    // seen at once), the two inflate streams low (long kernels that fill what is free), the main stream and the side stream
    // normal -- no class holds more than four streams even with two members on one device.  The copy stream, the side
    // stream and the inflaters' streams are made when first used (need_stream below).
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr;
    bool copy_pending = false;
    bool filter_pending = false;  // slimm_filter_alignments_launch ran; slimm_install_merged_partials completes it
    bool stream_ordered = false;  // slimm_set_stream_ordered: the caller enqueues its collectives on `stream`
    struct Staging {
        PinBuf<uint64_t> key;
        PinBuf<int32_t> ref, pos;
        PinBuf<uint16_t> flag;
        hipEvent_t done = nullptr;
        bool pending = false;
    } staging[2];

    uint32_t R = 0, T = 0;
    TileBucketing tiles;               // the bin tiles' layout, the plan of their bucketing and its tables (tile_bucketing.h)
    uint64_t Bp() const { return tiles.layout.Bp; }   // padded bins per coverage array (whole tiles)
    bool use_tiles() const { return tiles.plan.use_tiles; }   // LDS tile histograms (default) vs direct global atomics
    std::vector<uint32_t> bin_off_h;   // [R+1] padded offsets

    // static tables
    DevBuf<uint32_t> d_ref_len, d_bin_off, d_lin_dense;
    DevBuf<uint2> d_geo;              // {contig length, first bin} per reference: one gather in k_emit
    DevBuf<uint8_t> d_valid;
    DevBuf<uint4> d_rows16;           // per run: 16-byte lineage rows with the valid bit
    DevBuf<uint32_t> d_level_taxon;    // [(index << 3) | level] -> dense taxon (8 << taxon_shift entries)
    DevBuf<uint32_t> d_taxon_off, d_taxon_idx;  // ... and back: the (level, index) entries of dense taxon t (CSR)
    uint32_t taxon_shift = 0;
    uint32_t Tsel = 0;                 // size of the selectors' taxon space: 8 << taxon_shift (16-byte rows) or T
    PinBuf<uint4> h_rows16;
    DevBuf<uint32_t> d_valid_bits;     // one bit per reference: what k_filter_compact asks before anything else
    PinBuf<uint32_t> h_valid_bits;
    std::vector<uint32_t> valid_bits_prev;   // references whose bit is set in h_valid_bits
    bool rows16_base_ready = false;    // h_rows16 holds the static part of every row
    std::vector<uint32_t> rows16_prev; // references whose valid bit is set in h_rows16
    bool use_rows16 = false;
    bool ref16 = false;                // the targets' reference words are 16 bits wide (kernels.h: TargetRefs)
    // records
    DevBuf<uint64_t> in_key;
    DevBuf<int32_t> in_ref, in_pos;
    DevBuf<uint16_t> in_flag;
    DevBuf<uint32_t> in_check;     // slimm_push_records_checked: a second hash of every record's read name
    bool has_check = false;        // ... all pushed batches carry one (checked and unchecked pushes do not mix)
    bool packed = false;           // slimm_push_records_packed: 16 bytes per record, no flag array (forms do not mix)
    bool marked = false;           // slimm_push_records_marked: 8 bytes per record, no key array (grouped input only)
    WindowPipeline win;     // a file's bytes in windows, inflated and decoded on the device (windows.h, windows.hip)
    std::vector<slimm_ctx*> filter_peers;   // member 0 of a group: the other members (its record filter stats are the group's)
    DeviceRecords rec;      // what analyze reads (owned buffers or borrowed pointers)
    bool borrowed = false;
    uint64_t n_pushed = 0;
    // work arrays
    // record_order = ANY (group_by_ident.hip): the grouped stream {identity, {reference, bin}, check word} + scratch
    DevBuf<uint64_t> c_ident, s_ident;
    DevBuf<uint2> c_pay, s_pay;
    DevBuf<uint32_t> group_hist, c_chk, s_chk;
    DevBuf<uint32_t> tgt_ref, tgt_gbin;  // targets (top bit: first of its read / the read has one target), in slots;
                                         // tgt_ref holds uint16_t words when ref16 (target_refs())
    TargetRefs target_refs() const { return TargetRefs{tgt_ref.p, ref16}; }
    DevBuf<uint4> slots;                 // per kSlotRecs records: {first target, targets, reads, mapped records}
    bool keep_bins = true;       // materialise cov / uniq_cov / uniq_cov2 in HBM (slimm_keep_bins)
    bool binsA_stored = false, binsB_stored = false;
    DevBuf<uint32_t> sel;                               // per read, dense: its uniq_cov2 bin, Bp + LCA taxon, or 0xffffffff
    DevBuf<uint32_t> filter_redo;                       // slots k_filter_compact leaves to k_filter_walk
    DevBuf<uint32_t> slot_rbase, slot_bbase;            // reads in front of a slot = rbase[s] + bbase[s >> 10] (side stream)
    hipStream_t side_stream = nullptr;
    hipEvent_t front_done = nullptr, prefix_done = nullptr;
    bool prefix_pending = false;  // prefix_done has been recorded and not been waited for by the main stream yet
    // multi-GPU coverage summary [4R sums | 16 scalars | bitmaps]: n_slices = 0: not announced (bitmaps by extra kernels),
    // 1: bitmaps written by k_tile_hist as [cov | uniq_cov], n > 1: in n slices of tiles for the all-to-all exchange
    uint32_t summary_slices = 0;
    bool summary_has_bits = false;   // the bitmaps of this analysis are in `summary` already
    uint32_t summary_layout = 0xffffffffu;  // n_slices the buffer was last zeroed for
    DevBuf<uint32_t> d_sum_vec;      // all-to-all form: [4R | 16] additive vector, all-reduced in place
    uint32_t slice_tiles() const { return summary_slices > 1 ? (tiles.layout.ntiles + summary_slices - 1) / summary_slices : tiles.layout.ntiles; }
    uint64_t slice_words() const { return static_cast<uint64_t>(slice_tiles()) * (tiles.layout.tile_bins() / 32); }  // per array
    uint64_t summary_words() const { return 4ull * R + 16 + 2ull * std::max<uint32_t>(summary_slices, 1u) * slice_words(); }
    BitsLayout bits_layout() {
        BitsLayout b;
        if (summary_has_bits) {
            b.base = reinterpret_cast<uint64_t*>(summary.p + 4ull * R + 16);
            b.tps = slice_tiles();
            b.slice_w64 = slice_words() / 2;
        }
        return b;
    }
    bool statsA_final = false;  // k_pack has added the non-zero counts of the split tiles to the fused statistics
    bool bins_exposed = false;  // the caller holds the coverage buffer (may have merged other ranks' bins into it)
    DevBuf<uint32_t> bins;       // cov | uniq_cov | tail | uniq_cov2
    DevBuf<uint32_t> counters;   // CNT_WORDS
    DevBuf<uint32_t> ref_stats;  // [R*4] then [R*4]
    DevBuf<uint32_t> summary;    // multi-GPU: [4R sums | 16 scalars | cov bits | uniq_cov bits]
    DevBuf<uint32_t> lca_count, marks;
    DevBuf<uint32_t> d_partials;  // multi-GPU: the additive partial results, summed across ranks in place
    PinBuf<uint32_t> h_partials;
    DevBuf<uint64_t> pair_tab, pair_list;
    uint32_t pair_cap = 0;  // power of two
    // pinned staging
    PinBuf<uint32_t> h_stats, h_small, h_lca, h_marks;
    PinBuf<uint64_t> h_pairs;

    // per-run state
    bool analyzed = false, covered = false, filtered = false, counted = false, no_hits = false;
    uint32_t local_V = 0, local_M = 0, local_P = 0;
    uint32_t n_pairs = 0;
    std::vector<uint32_t> nz_ucov2;
    // partials handed out / installed
    std::vector<uint32_t> part_u2, part_lca, part_marks;
    std::vector<uint64_t> part_pairs;

    // kernel timing
    bool timing = false;
    int timing_only = -1;  // >= 0: bracket only this kernel id (keeps the event overhead out of the other launches)
    struct Ev {
        hipEvent_t a, b;
        int id;
    };
    std::vector<Ev> ev_used, ev_free;
    double k_ms[K_COUNT] = {0};
    uint32_t k_n[K_COUNT] = {0};

    // packed result blocks: A = [4R stats | 32 counters | 16 tail], B = [4R stats2 | 32 counters | R marks | T lca]
    size_t statsA_words() const { return 4ull * R + 64; }
    size_t statsB_words() const { return 5ull * R + 32 + T; }
    bool pair_clean = false;  // the (taxon, ref) hash set holds only empty slots
    uint32_t* cov() { return bins.p; }
    uint32_t* ucov() { return bins.p + Bp(); }
    uint32_t* tail() { return bins.p + 2 * Bp(); }
    uint32_t* ucov2() { return bins.p + 2 * Bp() + kTailWords; }
    uint32_t* lca_tiles() { return bins.p + 3 * Bp() + kTailWords; }  // [Tpad] right behind uniq_cov2: one index space
};

namespace slimm {

// SLIMM_TRACE=host: wall-clock marks of the host steps between the two device phases, on stderr
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    const char* what;
    explicit HostTrace(const char* w) : on(false), what(w) {
        static const bool enabled = traced("host");
        on = enabled;
        if (on) t0 = std::chrono::steady_clock::now();
    }
    void mark(const char* step) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[host] %s: %s %.1f us\n", what, step, std::chrono::duration<double, std::micro>(t1 - t0).count());
        t0 = t1;
    }
};

int fail(slimm_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail((c), SLIMM_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define SLIMM_TRY(expr)                      \
    do {                                     \
        const int rc_ = (expr);              \
        if (rc_ != SLIMM_OK) return rc_;     \
    } while (0)

struct KernelTimer {  // brackets one launch (or a group) with events when timing is on
    slimm_ctx* c;
    slimm_ctx::Ev ev{};
    bool on;
    bool dispatch;  // the events are handed to the launch itself (hipExtLaunchKernelGGL: the dispatch's own time stamps)
    KernelTimer(slimm_ctx* ctx, int id, bool of_dispatch = false)
        : c(ctx), on(ctx->timing && (ctx->timing_only < 0 || ctx->timing_only == id)), dispatch(of_dispatch) {
        if (!on) return;
        if (!c->ev_free.empty()) {
            ev = c->ev_free.back();
            c->ev_free.pop_back();
        } else {
            (void)hipEventCreate(&ev.a);
            (void)hipEventCreate(&ev.b);
        }
        ev.id = id;
        if (!dispatch) (void)hipEventRecord(ev.a, c->stream);
    }
    hipEvent_t t0() const { return on ? ev.a : nullptr; }
    hipEvent_t t1() const { return on ? ev.b : nullptr; }
    ~KernelTimer() {
        if (!on) return;
        if (!dispatch) (void)hipEventRecord(ev.b, c->stream);
        c->ev_used.push_back(ev);
    }
};

void drain_events(slimm_ctx* c);
int ensure_work_buffers(slimm_ctx* c, uint32_t n);
int ensure_pair_table(slimm_ctx* c, uint32_t cap);
int check_device_errors(slimm_ctx* c, uint32_t err);
// records.hip: c->rec = the owned record arrays in_* from record `from` on, in the file's form (marked / packed / has_check)
void view_records(slimm_ctx* c, uint64_t from = 0);

enum StreamClass { kStreamHigh = 0, kStreamNormal = 1, kStreamLow = 2 };
inline hipError_t need_stream(hipStream_t& s, StreamClass cls = kStreamNormal) {
    if (s) return hipSuccess;
    int least = 0, greatest = 0;  // (numerically: greatest priority = the smallest number)
    if (cls == kStreamNormal || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest)
        return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, cls == kStreamHigh ? greatest : least);
}

// Grows one record array to `cap` elements, keeping the `used` elements pushed so far (when the array holds them at all:
// an array the file's record form does not use is neither allocated nor copied).
// later != nullptr: no hipFree now (it waits for every kernel in flight -- the inflate of the windows behind this one):
// what the array was goes there and is freed when the file has ended
template <typename T>
hipError_t grow_record_array(DevBuf<T>& buf, uint64_t cap, uint64_t used, hipStream_t st, std::vector<void*>* later = nullptr) {
    if (cap <= buf.cap) return hipSuccess;
    if (used == 0 || buf.cap < used) return later ? buf.ensure_later(cap, *later) : buf.ensure(cap);  // nothing of this file in it
    return buf.grow_keeping(cap, 0, used, st, true, later);
}

}  // namespace slimm
