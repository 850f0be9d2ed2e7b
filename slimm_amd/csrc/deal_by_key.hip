// A stable partition of four-array records by owner, owner = (key & kKeyMask) % m: how a group gives every read of a file
// in no particular order to ONE member without the host (include/slimm_hip.h, slimm_partition_by_key; group.hip).  The rule
// is the host dealing's (group.hip: deal), bit for bit, and the order inside an owner's stretch is the input order: the
// first record of a (read, reference) in FILE order decides its bin (reference src/read_stat.hpp:116-135), so the members
// must see their reads' records in the order one context would.
//
// Shaped like the counting passes of group_by_ident.hip: kDealGrid persistent workgroups, each owning one contiguous stretch
// of the input, and three steps -- count per (workgroup, owner), scan the counts owner-major, scatter.  A workgroup is ONE
// wave: it walks its stretch in rounds of kDealRound records (kDealItems loads per lane in flight), and inside a wave the
// rank of a record among its owner's comes from a ballot per owner present (a loop over the distinct owners, the next one
// read from the first lane left), the owner's cursor from LDS.  No atomics anywhere, nothing depends on timing.  The owner
// is reduced in 32-bit steps ((hi % m) * (2^32 % m) + lo % m) % m: m is any number up to 255 and a 64-bit remainder is a
// long software sequence.  The pass is bound by memory: 8 bytes read per record to count, 22 read + 22 written to scatter.
#include "context.h"
#include "deal_by_key.h"

namespace slimm {
namespace {

__device__ __forceinline__ uint32_t deal_owner(uint64_t key, uint32_t m, uint32_t c32) {
    const uint32_t lo = static_cast<uint32_t>(key), hi = static_cast<uint32_t>(key >> 32) & 0x3fffffffu;  // (kKeyMask: 62 bits)
    return ((hi % m) * c32 + lo % m) % m;
}

// f(owner, lanes) once per distinct owner among the wave's live lanes (wave-uniform arguments), lowest lane first
template <typename F>
__device__ __forceinline__ void deal_each_owner(uint32_t owner, bool live, F&& f) {
    uint64_t todo = __builtin_amdgcn_ballot_w64(live);
    while (todo) {
        const uint32_t o = __builtin_amdgcn_readlane(owner, static_cast<uint32_t>(__builtin_ctzll(todo)));
        const uint64_t mine = __builtin_amdgcn_ballot_w64(live && owner == o);
        f(o, mine);
        todo &= ~mine;
    }
}

__device__ __forceinline__ uint64_t deal_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ void deal_stretch_of(uint64_t n, uint64_t per, uint64_t& lo, uint64_t& hi) {
    lo = deal_min(n, static_cast<uint64_t>(blockIdx.x) * per);
    hi = deal_min(n, lo + per);
}

// matrix[owner * kDealGrid + workgroup] = records of the workgroup's stretch with that owner
__global__ __launch_bounds__(64) void k_deal_count(const uint64_t* __restrict__ key, uint64_t n, uint64_t per, uint32_t m, uint32_t c32,
                                                   uint32_t* __restrict__ matrix) {
    __shared__ uint32_t s_h[kDealMaxOwners + 1];
    const uint32_t lane = threadIdx.x;
    for (uint32_t o = lane; o < m; o += 64u) s_h[o] = 0u;
    __syncthreads();
    uint64_t lo, hi;
    deal_stretch_of(n, per, lo, hi);
    for (uint64_t r0 = lo; r0 < hi; r0 += kDealRound) {
        uint64_t k[kDealItems];
#pragma unroll
        for (uint32_t u = 0; u < kDealItems; ++u) k[u] = key[deal_min(r0 + u * 64u + lane, hi - 1u)];  // (clamped: all loads in flight at once)
#pragma unroll
        for (uint32_t u = 0; u < kDealItems; ++u) {
            const bool live = r0 + u * 64u + lane < hi;
            deal_each_owner(deal_owner(k[u], m, c32), live, [&](uint32_t o, uint64_t mine) {
                if (lane == 0u) s_h[o] += static_cast<uint32_t>(__popcll(mine));
            });
        }
    }
    __syncthreads();
    for (uint32_t o = lane; o < m; o += 64u) matrix[static_cast<size_t>(o) * kDealGrid + blockIdx.x] = s_h[o];
}

// the matrix's exclusive prefix in place, owner-major (all of owner 0's workgroups, then owner 1's ...): where every
// (owner, workgroup) starts writing; counts[o] = owner o's records.  One workgroup, a contiguous chunk per thread
__global__ __launch_bounds__(1024) void k_deal_scan(uint32_t* matrix, uint32_t m, uint64_t n, uint64_t* __restrict__ counts) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t E = m * kDealGrid, chunk = (E + 1023u) / 1024u;
    const uint32_t lo = min(E, tid * chunk), hi = min(E, lo + chunk);
    uint32_t sum = 0;
    for (uint32_t e = lo; e < hi; ++e) sum += matrix[e];
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(inc, o, 64);
        if (lane >= static_cast<uint32_t>(o)) inc += a;
    }
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t w = 0; w < 16u; ++w) run += w < wave ? s_w[w] : 0u;
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t v = matrix[e];
        matrix[e] = run;
        run += v;
    }
    __threadfence_block();
    __syncthreads();
    for (uint32_t o = tid; o < m; o += 1024u)
        counts[o] = (o + 1u < m ? matrix[static_cast<size_t>(o + 1u) * kDealGrid] : n) - matrix[static_cast<size_t>(o) * kDealGrid];
}

// every record to its owner's stretch: cursor of (owner, this workgroup) + records of that owner in front of it in the
// workgroup's stretch -- rounds, loads and owners' lanes in order, so input order is kept
template <bool kCheck>
__global__ __launch_bounds__(64) void k_deal_scatter(const DealRecords in, uint64_t n, uint64_t per, uint32_t m, uint32_t c32,
                                                     const uint32_t* __restrict__ matrix, const DealRecords out) {
    __shared__ uint32_t s_cur[kDealMaxOwners + 1];
    const uint32_t lane = threadIdx.x;
    for (uint32_t o = lane; o < m; o += 64u) s_cur[o] = matrix[static_cast<size_t>(o) * kDealGrid + blockIdx.x];
    __syncthreads();
    uint64_t lo, hi;
    deal_stretch_of(n, per, lo, hi);
    for (uint64_t r0 = lo; r0 < hi; r0 += kDealRound) {
        uint64_t k[kDealItems];
        int32_t r[kDealItems], p[kDealItems];
        uint32_t f[kDealItems], c[kDealItems];
#pragma unroll
        for (uint32_t u = 0; u < kDealItems; ++u) {
            const uint64_t i = deal_min(r0 + u * 64u + lane, hi - 1u);
            k[u] = in.key[i];
            r[u] = in.ref[i];
            p[u] = in.pos[i];
            f[u] = in.flag[i];
            c[u] = kCheck ? in.check[i] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kDealItems; ++u) {
            const bool live = r0 + u * 64u + lane < hi;
            const uint32_t owner = deal_owner(k[u], m, c32);
            uint32_t dst = 0;
            deal_each_owner(owner, live, [&](uint32_t o, uint64_t mine) {
                const uint32_t base = s_cur[o];
                __builtin_amdgcn_wave_barrier();   // (every lane has read the cursor before lane 0 moves it)
                if (lane == 0u) s_cur[o] = base + static_cast<uint32_t>(__popcll(mine));
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mine >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mine), 0u));
                if (owner == o) dst = base + below;
            });
            if (live && dst < n) {   // (dst < n by construction: nothing is ever written outside the arrays)
                out.key[dst] = k[u];
                out.ref[dst] = r[u];
                out.pos[dst] = p[u];
                out.flag[dst] = static_cast<uint16_t>(f[u]);
                if (kCheck) out.check[dst] = c[u];
            }
        }
    }
}

}  // namespace

void launch_deal_by_key(hipStream_t st, const DealRecords& in, uint64_t n, uint32_t m, const DealRecords& out, uint32_t* matrix,
                        uint64_t* counts) {
    const uint64_t per = deal_stretch(n);
    const uint32_t c32 = static_cast<uint32_t>((1ull << 32) % m);
    hipLaunchKernelGGL(k_deal_count, dim3(kDealGrid), dim3(64), 0, st, static_cast<const uint64_t*>(in.key), n, per, m, c32, matrix);
    hipLaunchKernelGGL(k_deal_scan, dim3(1), dim3(1024), 0, st, matrix, m, n, counts);
    if (in.check && out.check)
        hipLaunchKernelGGL(k_deal_scatter<true>, dim3(kDealGrid), dim3(64), 0, st, in, n, per, m, c32, static_cast<const uint32_t*>(matrix), out);
    else
        hipLaunchKernelGGL(k_deal_scatter<false>, dim3(kDealGrid), dim3(64), 0, st, in, n, per, m, c32, static_cast<const uint32_t*>(matrix), out);
}

namespace {

struct DealBuffers {   // one member's records as it partitioned them, and the kernels' scratch
    int device = -1;
    DevBuf<uint64_t> key, counts;
    DevBuf<int32_t> ref, pos;
    DevBuf<uint16_t> flag;
    DevBuf<uint32_t> check, matrix;
    hipError_t ensure(uint64_t n, uint32_t m, bool with_check) {
        hipError_t e = key.ensure(n);
        if (e == hipSuccess) e = ref.ensure(n);
        if (e == hipSuccess) e = pos.ensure(n);
        if (e == hipSuccess) e = flag.ensure(n);
        if (e == hipSuccess && with_check) e = check.ensure(n);
        if (e == hipSuccess) e = matrix.ensure(deal_matrix_words(m));
        if (e == hipSuccess) e = counts.ensure(m);
        return e;
    }
    DealRecords records() const {
        DealRecords r;
        r.key = key.p, r.ref = ref.p, r.pos = pos.p, r.flag = flag.p, r.check = check.p;
        return r;
    }
    ~DealBuffers() {
        if (device >= 0) (void)hipSetDevice(device);
    }
};

template <typename T>
hipError_t deal_copy(slimm_ctx* dst, T* to, slimm_ctx* src, const T* from, uint64_t n) {
    if (dst->device == src->device) return hipMemcpyAsync(to, from, n * sizeof(T), hipMemcpyDeviceToDevice, dst->stream);
    return hipMemcpyPeerAsync(to, dst->device, from, src->device, n * sizeof(T), dst->stream);
}

}  // namespace

int deal_by_key(slimm_ctx* const* members, uint32_t m, uint64_t* held, uint64_t* own, uint32_t* failed) {
    if (!members || !m || m > kDealMaxOwners || !held || !own || !failed) return SLIMM_E_INVALID;
    bool any = false, with_check = false;
    for (uint32_t i = 0; i < m; ++i) {
        slimm_ctx* c = members[i];
        *failed = i;
        if (!c) return SLIMM_E_INVALID;
        if (c->device < 0) return fail(c, SLIMM_E_INVALID, "host-only context has no record stream");
        if (c->analyzed) return fail(c, SLIMM_E_INVALID, "records already analysed; reset first");
        if (c->win.file.active && !c->win.file.closed) return fail(c, SLIMM_E_INVALID, "the file's last window has not been pushed");
        if (!c->n_pushed) continue;
        if (c->borrowed || c->marked || c->packed)
            return fail(c, SLIMM_E_INVALID, "records are dealt by key in the four-array form, from the context's own arrays");
        if (any && with_check != c->has_check) return fail(c, SLIMM_E_INVALID, "the members' records carry check words or none, all alike");
        any = true;
        with_check = c->has_check;
    }
    // ---- every member partitions its own records (the devices side by side), the stretch lengths come to the host
    std::vector<DealBuffers> send(m);
    std::vector<uint64_t> cnt(static_cast<size_t>(m) * m, 0);   // cnt[i * m + o]: member i's records that member o owns
    for (uint32_t i = 0; i < m; ++i) {
        slimm_ctx* c = members[i];
        *failed = i;
        const uint64_t n = c->n_pushed;
        if (!n) continue;
        (void)hipSetDevice(c->device);
        if (c->copy_pending) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->copy_done, 0));
        send[i].device = c->device;
        HIP_TRY(c, send[i].ensure(n, m, with_check));
        DealRecords in;
        in.key = c->in_key.p, in.ref = c->in_ref.p, in.pos = c->in_pos.p, in.flag = c->in_flag.p, in.check = with_check ? c->in_check.p : nullptr;
        launch_deal_by_key(c->stream, in, n, m, send[i].records(), send[i].matrix.p, send[i].counts.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&cnt[static_cast<size_t>(i) * m], send[i].counts.p, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    for (uint32_t i = 0; i < m; ++i) {
        *failed = i;
        (void)hipSetDevice(members[i]->device);
        HIP_TRY(members[i], hipStreamSynchronize(members[i]->stream));
    }
    std::vector<uint64_t> total(m, 0);
    for (uint32_t j = 0; j < m; ++j) {
        for (uint32_t i = 0; i < m; ++i) total[j] += cnt[static_cast<size_t>(i) * m + j];
        *failed = j;
        if (total[j] >= record_cap()) return fail(members[j], SLIMM_E_INVALID, "a context handles fewer than 2^31 records; shard the stream");
    }
    // ---- member j takes stretch j of every member, in member order: the file's order inside every destination
    for (uint32_t j = 0; j < m; ++j) {
        slimm_ctx* c = members[j];
        *failed = j;
        (void)hipSetDevice(c->device);
        own[j] = 0;
        if (!any) continue;
        c->n_pushed = 0;   // (its records are in its send buffers: the arrays are free)
        c->marked = c->packed = false;
        c->has_check = with_check;
        SLIMM_TRY(slimm_reserve(c, total[j]));
        if (total[j]) {
            HIP_TRY(c, c->in_flag.ensure(c->in_key.cap));
            if (with_check) HIP_TRY(c, c->in_check.ensure(c->in_key.cap));
        }
        uint64_t at = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const uint64_t* row = &cnt[static_cast<size_t>(i) * m];
            const uint64_t k = row[j];
            if (!k) continue;
            uint64_t from = 0;
            for (uint32_t o = 0; o < j; ++o) from += row[o];
            const DealBuffers& s = send[i];
            HIP_TRY(c, deal_copy(c, c->in_key.p + at, members[i], s.key.p + from, k));
            HIP_TRY(c, deal_copy(c, c->in_ref.p + at, members[i], s.ref.p + from, k));
            HIP_TRY(c, deal_copy(c, c->in_pos.p + at, members[i], s.pos.p + from, k));
            HIP_TRY(c, deal_copy(c, c->in_flag.p + at, members[i], s.flag.p + from, k));
            if (with_check) HIP_TRY(c, deal_copy(c, c->in_check.p + at, members[i], s.check.p + from, k));
            if (i == j) own[j] = k;
            at += k;
        }
    }
    for (uint32_t j = 0; j < m; ++j) {   // (the send buffers go when every copy out of them is done)
        slimm_ctx* c = members[j];
        *failed = j;
        (void)hipSetDevice(c->device);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (any) {
            c->n_pushed = total[j];
            view_records(c);
        }
        held[j] = c->n_pushed;
    }
    return SLIMM_OK;
}

}  // namespace slimm

// The partition by itself, host arrays in and out (include/slimm_hip.h): the kernels the group runs, timed
extern "C" int slimm_partition_by_key(int device, const uint64_t* key, const int32_t* ref, const int32_t* pos, const uint16_t* flag,
                                      const uint32_t* check, uint64_t n, uint32_t m, uint64_t* key_out, int32_t* ref_out, int32_t* pos_out,
                                      uint16_t* flag_out, uint32_t* check_out, uint64_t* counts_out, double* kernel_ms, char* err,
                                      uint64_t err_cap) {
    auto fail = [&](int code, const std::string& why) {
        if (err && err_cap) {
            const size_t k = std::min<size_t>(why.size(), err_cap - 1);
            memcpy(err, why.data(), k);
            err[k] = 0;
        }
        return code;
    };
    if (kernel_ms) *kernel_ms = 0;
    if (!m || m > slimm::kDealMaxOwners) return fail(-1, "1 .. 255 members");
    if (!counts_out) return fail(-1, "null argument");
    if (n && (!key || !ref || !pos || !flag || !key_out || !ref_out || !pos_out || !flag_out)) return fail(-1, "null argument");
    if (n >= (1ull << 31)) return fail(-1, "fewer than 2^31 records");
    const bool with_check = check && check_out;
    if (hipSetDevice(device) != hipSuccess) return fail(-2, "hipSetDevice failed");
    slimm::DealBuffers in, out;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    std::string msg;
    auto ok = [&](hipError_t e, const char* what) {
        if (e == hipSuccess || rc) return;
        rc = -2;
        msg = std::string(what) + ": " + hipGetErrorString(e);
    };
    const uint64_t room = std::max<uint64_t>(n, 1u);
    ok(in.ensure(room, m, with_check), "hipMalloc");
    ok(out.ensure(room, m, with_check), "hipMalloc");
    if (!rc && n) {
        ok(hipMemcpy(in.key.p, key, n * 8, hipMemcpyHostToDevice), "hipMemcpy");
        ok(hipMemcpy(in.ref.p, ref, n * 4, hipMemcpyHostToDevice), "hipMemcpy");
        ok(hipMemcpy(in.pos.p, pos, n * 4, hipMemcpyHostToDevice), "hipMemcpy");
        ok(hipMemcpy(in.flag.p, flag, n * 2, hipMemcpyHostToDevice), "hipMemcpy");
        if (with_check) ok(hipMemcpy(in.check.p, check, n * 4, hipMemcpyHostToDevice), "hipMemcpy");
    }
    ok(hipEventCreate(&e0), "hipEventCreate");
    ok(hipEventCreate(&e1), "hipEventCreate");
    if (!rc) {
        ok(hipEventRecord(e0, nullptr), "hipEventRecord");
        slimm::launch_deal_by_key(nullptr, in.records(), n, m, out.records(), in.matrix.p, in.counts.p);
        ok(hipGetLastError(), "launch");
        ok(hipEventRecord(e1, nullptr), "hipEventRecord");
        ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        float ms = 0;
        if (!rc && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && kernel_ms) *kernel_ms = ms;
        ok(hipMemcpy(counts_out, in.counts.p, m * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
        if (n) {
            ok(hipMemcpy(key_out, out.key.p, n * 8, hipMemcpyDeviceToHost), "hipMemcpy");
            ok(hipMemcpy(ref_out, out.ref.p, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
            ok(hipMemcpy(pos_out, out.pos.p, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
            ok(hipMemcpy(flag_out, out.flag.p, n * 2, hipMemcpyDeviceToHost), "hipMemcpy");
            if (with_check) ok(hipMemcpy(check_out, out.check.p, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc ? fail(rc, msg) : 0;
}
