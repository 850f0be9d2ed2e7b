// Internal to the library: the per-member steps of slimm_group_stitch_ranges (group.hip drives them on opaque contexts,
// split.hip holds them) -- one file split by byte range over a group's members (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE
// RANGE").  The steps here know no codec: what a streamed codec adds to the stitch is its row of kCodecs (windows.h:
// StreamCodec -- whether a range must be announced, the stitch hook and its words), and the check itself lies beside the
// decoder that owns the state it reads.  Every step finishes its own device work before it returns: the next step may run on
// another member's device.
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
// The stitch hook of MEMBER 0's codec over all the members, once, before any text is joined (none: SLIMM_OK).  SLIMM_OK, or the
// code with the message on member *bad; *split_words wraps SLIMM_E_SPLIT (member, message), *noun is member_failed's
int split_codec_stitch(slimm_ctx* const* members, uint32_t n, uint32_t* bad, const char** split_words, const char** noun);
// ... and its hook between the members' two passes (slimm_group_gzip_windows); a codec that has none is refused by gzip's
int split_codec_windows(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
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
