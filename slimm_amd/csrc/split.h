// Internal to the library: the per-member steps of slimm_group_stitch_ranges (group.hip drives them, split.hip holds them)
// -- one file (BAM, SAM, BGZF SAM, bzip2 SAM, zstd SAM, xz SAM) split by byte range over a group's members (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE").
// Every step finishes its own device work before it returns: the next step may run on another member's device.
#pragma once
#include <stdint.h>

#include "../../include/slimm_hip.h"

namespace slimm {

struct SplitRange {
    bool found_start = false;   // the range holds a record start (false: all its bytes are head)
    uint64_t head_len = 0;      // bytes in front of its first record
    uint64_t n_records = 0;     // records decoded so far
};
int split_range(slimm_ctx* c, SplitRange* out);
// bzip2 SAM: the members' block chains against each other, left to right, on host scalars (before any text is joined):
// every chain ends at the bit where the next member that holds an element starts, that member's blocks fit the stream's
// level, and the combined CRC of a stream over a cut is its marker's.  SLIMM_OK, or the code with the message on member *bad
bool split_is_bzip2(const slimm_ctx* c);
int split_bz2_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// zstd SAM: left to right on host scalars, every member's decoder stands between frames at its range's end with every byte of
// the range read.  SLIMM_OK, or SLIMM_E_SPLIT with the message on member *bad
bool split_is_zstd(const slimm_ctx* c);
int split_zstd_ends(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// xz SAM: left to right on host scalars, every member's walker stands at its range's end with every byte of the range read; a
// member that was told a check kind has a stream over the cut in front of it, of that kind; the blocks of such a stream in
// the ranges on the left are, in order and in number, the index records that the member which met the index kept (those in
// front of its own blocks' records).  SLIMM_OK, or the code with the message on member *bad
bool split_is_xz(const slimm_ctx* c);
int split_xz_streams(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// gzip SAM.  split_gz_windows, between the members' window pass and their text pass (slimm_group_gzip_windows), left to right:
// member k's chain ended on member k + 1's first bit; its final 16-bit window, resolved against the bytes in front of its
// own range (a tiny kernel on its device), becomes the 32 768 bytes in front of member k + 1's, copied device to device, with
// how many of them belong to the open gzip member; then every member's file state is fresh for the text pass, its
// announcements kept.  split_gz_chains, in the stitch on host scalars: every chain ended on its range's end and the text pass
// reproduced the window pass's end bit and text length (SLIMM_E_SPLIT), and the CRC register and length of a gzip member
// that lies over cuts, folded left to right, are its trailer's (SLIMM_E_INVALID, the single context's words)
bool split_is_gzip(const slimm_ctx* c);
int split_gz_windows(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
int split_gz_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// the head of `right` as one more window of `left` (final: it must end with a complete record, else SLIMM_E_SPLIT)
int split_append_head(slimm_ctx* left, slimm_ctx* right, bool final, uint64_t* n_records);
// `right`'s first record against the last record of `left` (its carry): the same name clears the run-start bit and
// corrects right's Q18 counts
int split_join(slimm_ctx* left, slimm_ctx* right);
// the index of the first record that starts a run (the record count when none does)
int split_first_start(slimm_ctx* c, uint64_t* index);
// records [0, n) of src appended to dst, device to device
int split_take(slimm_ctx* dst, slimm_ctx* src, uint64_t n);
// the member's records are [from, its count) from now on; its Q18 counts are the group's business
int split_keep(slimm_ctx* c, uint64_t from);
// (not a step of the stitch: when the group is made) member 0 answers slimm_get_record_filter_stats with the sum over the
// members, whichever of them decoded a record
void group_filter_peers(slimm_ctx* member0, slimm_ctx* const* others, uint32_t n);

}  // namespace slimm
