// Internal to the library: the stable partition of four-array records by owner (deal_by_key.hip) -- how a group gives
// every read of a file in no particular order to one member on the device (group.hip: deal_by_key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct slimm_ctx;

namespace slimm {

// A fixed number of persistent workgroups of one wave each; every one owns one contiguous stretch of the input, a whole
// number of rounds of kDealRound records (64 lanes x kDealItems records in flight per lane).
constexpr uint32_t kDealGrid = 2048;
constexpr uint32_t kDealItems = 8;
constexpr uint32_t kDealRound = 64 * kDealItems;
constexpr uint32_t kDealMaxOwners = 255;

struct DealRecords {   // device arrays; check may be null (in and out alike)
    uint64_t* key = nullptr;
    int32_t *ref = nullptr, *pos = nullptr;
    uint16_t* flag = nullptr;
    uint32_t* check = nullptr;
};

// records of a workgroup's stretch for n records in all
inline uint64_t deal_stretch(uint64_t n) {
    const uint64_t per = (n + kDealGrid - 1) / kDealGrid;
    return (per + kDealRound - 1) / kDealRound * kDealRound;
}
// 32-bit words of the count matrix the three steps share: [owner][workgroup]
inline size_t deal_matrix_words(uint32_t m) { return static_cast<size_t>(m) * kDealGrid; }

// out = the n records of in, reordered into m stretches, stretch o = the records with (key & kKeyMask) % m == o in input
// order; counts[o] = its length.  matrix: deal_matrix_words(m) words of scratch.  n < 2^32, 1 <= m <= kDealMaxOwners.
// Three launches on st: count per (workgroup, owner), scan owner-major, scatter.
void launch_deal_by_key(hipStream_t st, const DealRecords& in, uint64_t n, uint32_t m, const DealRecords& out, uint32_t* matrix,
                        uint64_t* counts);

// The members' four-array records dealt by key (slimm_group_get_profiles, slimm_group_stitch_ranges): every member
// partitions its own records, member j then holds stretch j of every member in member order -- copied device to device into
// its own record arrays, which the send buffers (one more copy of the records, 22 bytes each) have freed by then; the send
// buffers are released before this returns.  held[j]: the records member j holds afterwards, own[j]: those of them it had
// itself.  Every member's stream is idle on return.  An error is the error of member *failed.
int deal_by_key(slimm_ctx* const* members, uint32_t m, uint64_t* held, uint64_t* own, uint32_t* failed);

}  // namespace slimm
