/* ============================================================================
 * slimm_hip.h -- C ABI of the MI355X-native SLIMM alignment-to-profile path.
 *
 * The reference (seqan/slimm) has no plugin/FFI interface; the seam this library replaces is
 * the trio of `class slimm` member calls made by slimm::get_profiles()
 * (reference src/slimm.hpp:449 analyze_alignments, :464 filter_alignments,
 * :485 get_reads_lca_count, :489 write_abundance) and the public members they communicate
 * through (src/slimm.hpp:103-127).  Each entry point below names the reference code it stands for.
 *
 * Conventions: plain pointers and sizes, no C++ types, no exceptions across the boundary.
 * Every function returning int returns SLIMM_OK (0) or a negative SLIMM_E_* code;
 * slimm_last_error() gives the text.  A context is NOT thread-safe (the reference object is
 * single-threaded, one `slimm` per process: src/slimm.hpp:946-958); use one context per GPU.
 * All `const` host arrays passed in are copied before the call returns; the caller keeps
 * ownership.  Device work runs on a stream owned by the context; every call that returns
 * host-visible results has synchronised that stream.
 * ==========================================================================*/
#ifndef SLIMM_HIP_H
#define SLIMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMM_LINEAGE_LEN 8 /* reference src/misc.hpp:4 LINAGE_LENGTH */

enum {
    SLIMM_OK = 0,
    SLIMM_E_INVALID = -1,   /* bad argument / call order */
    SLIMM_E_HIP = -2,       /* HIP runtime error (no GPU, out of memory, ...) */
    SLIMM_E_REF_RANGE = -3, /* a record names ref_id >= n_refs (undefined behaviour in the reference) */
    SLIMM_E_RUN_LENGTH = -4,/* (not returned any more: a read may have any number of alignment records; the value is
                               kept so that the codes after it do not move) */
    SLIMM_E_KEY_COLLISION = -5, /* records with one read key carry different check words (slimm_push_records_checked) */
    SLIMM_E_REGROUP = -6,   /* a GROUPED stream holds names ending in ".1" / ".2" without a mate flag whose flagged namesakes
                               may lie elsewhere in the file (quirk Q18): push the file again to a SLIMM_ORDER_ANY context */
    SLIMM_E_SPLIT = -7,     /* slimm_group_stitch_ranges: a member's guess of its first record was wrong (or its range could
                               not be joined to the one before): read the file through one member instead */
    SLIMM_E_RETRY = 2,      /* not an error: slimm_install_merged_partials asks for slimm_filter_alignments_launch again */
    SLIMM_E_NO_HITS = 1     /* not an error: no mapped record (reference prints a warning and writes nothing, src/slimm.hpp:451-455) */
};

/* Order of the record stream (SAM @HD SO:/GO: tags).  GROUPED = all records of one read name are
 * contiguous (mapper output order, `GO:query` / `SO:queryname`); ANY = no assumption (the reference
 * accepts any order because it groups through a hash map, src/slimm.hpp:204-211) -- the records are
 * then stably sorted by read identity on the device first. */
enum { SLIMM_ORDER_GROUPED = 0, SLIMM_ORDER_ANY = 1 };

/* Taxonomic ranks, reference src/misc.hpp:24-35. */
enum {
    SLIMM_RANK_STRAIN = 0, SLIMM_RANK_SPECIES, SLIMM_RANK_GENUS, SLIMM_RANK_FAMILY, SLIMM_RANK_ORDER,
    SLIMM_RANK_CLASS, SLIMM_RANK_PHYLUM, SLIMM_RANK_SUPERKINGDOM, SLIMM_RANK_INTERMEDIATE
};

typedef struct slimm_ctx slimm_ctx;

/* What slimm::get_profiles() knows before the record loop starts (src/slimm.hpp:409-445) plus
 * the arg_options the path reads (src/slimm.hpp:49-87). */
typedef struct {
    uint32_t n_refs;          /* header contigs, index = BAM refID */
    const uint32_t* ref_len;  /* [n_refs] contig lengths */
    const uint32_t* lineage;  /* [n_refs*8] taxids per contig: own, species, genus, family, order, class, phylum,
                                 superkingdom = db.ac__taxid[accession]; all-zero row for an accession missing from the
                                 database (src/slimm.hpp:433-442) */
    uint32_t bin_width;       /* -w; 0 = use avg_read_len (src/slimm.hpp:412-413) */
    uint32_t avg_read_len;    /* get_avg_read_length() of the input (src/misc.hpp:509-522) */
    uint32_t min_reads;       /* -mr; 0 = derive 1+(matches-1)/10000 (src/slimm.hpp:458-459); a statistic only */
    float cov_cut_off;        /* -cc quantile (default 0.95) */
    float abundance_cut_off;  /* -ac (default 0.01) */
    const char* rank;         /* -r: "species" (default), "genus", "family", "order", "class", "phylum" */
    /* db.taxid__name (src/misc.hpp:84): rank and name per taxid; taxids not listed read as (strain, "") like the
       reference's default-constructed map entry (src/slimm.hpp:565). */
    uint32_t n_taxa;
    const uint32_t* tax_id;   /* [n_taxa] */
    const uint32_t* tax_rank; /* [n_taxa] SLIMM_RANK_* */
    const char* const* tax_name; /* [n_taxa] NUL-terminated */
    int device;               /* HIP device ordinal */
    int record_order;         /* SLIMM_ORDER_* */
} slimm_config;

/* slimm::slimm(options) + the per-file reference initialisation of get_profiles() (src/slimm.hpp:96-101, 420-445). */
int slimm_create(const slimm_config* cfg, slimm_ctx** out);
void slimm_destroy(slimm_ctx* ctx);
const char* slimm_last_error(const slimm_ctx* ctx); /* ctx may be NULL: error of the calling thread's last failed slimm_create */

/* slimm::reset() (src/slimm.hpp:167-188): forget records and results, keep configuration, allocations and --
 * like the reference -- the cached cut-offs (quirk Q8: they survive reset in -d mode). */
int slimm_reset(slimm_ctx* ctx);
/* Clears the cached cut-offs and the derived min_reads as well (a fresh `slimm` object). */
int slimm_reset_cutoffs(slimm_ctx* ctx);

/* The cached cut-offs (src/slimm.hpp:155-156).  In the reference's -d mode one `slimm` object serves all files, so
 * files 2+ reuse file 1's cut-offs (Q8); a host that creates one context per file carries them over with these. */
int slimm_get_cutoff_cache(slimm_ctx* ctx, float* coverage_cut_off, float* uniq_coverage_cut_off);
int slimm_set_cutoff_cache(slimm_ctx* ctx, float coverage_cut_off, float uniq_coverage_cut_off);
/* options.min_reads as an earlier file left it: with -mr 0 the first file with mapped reads derives it INTO the options
 * (src/slimm.hpp:458-459), where it stays for the files behind it (Q8).  slimm_reset keeps the derived value like
 * slimm::reset() does, slimm_reset_cutoffs restores the configured one; a host with one context per file carries it over
 * with this (slimm_stats.min_reads of the file before). */
int slimm_set_min_reads(slimm_ctx* ctx, uint32_t min_reads);

/* ---- record stream: what the loop of analyze_alignments() reads from each BamAlignmentRecord
 *      (src/slimm.hpp:194-211): qName identity, flag, rID, beginPos; file order. ------------------
 * read_key: identity of the qName (equal names <=> equal keys); only the low 62 bits are significant
 * (the mate number from flag 0x40/0x80 is folded into the two low bits on the device).  The reference's key is the
 * string qName + ".1" / ".2" / nothing (src/slimm.hpp:204-208): an UNFLAGGED record whose name ends in ".1" / ".2" is
 * the same read as a first / last-in-pair record of the name without that suffix (Q18).  A producer that wants that
 * input class reproduced keys such a record by the shortened name and sets the mate bit in the flag it passes:
 * slimm_host_canonical_read_name below does it, and the library's own readers do.  The library compares
 * keys, never names: "equal names <=> equal keys" is the caller's promise.  GROUPED streams only ever compare
 * ADJACENT records, so a producer that hashes names can make the promise exact by comparing every name with the
 * one before it (the slimm command's reader does: host/alignment_file.cpp, separate_adjacent_names); for ANY order
 * a 62-bit hash leaves ~n^2 / 2^63 odds of two different names meeting.
 *
 * Q18 ON A GROUPED STREAM.  A file grouped by QNAME (mapper output, @HD GO:query / SO:queryname) keeps the records of one
 * QNAME adjacent -- not the records of one reference KEY STRING: `r` (flag 0x40) and the unflagged `r.1` are one read of
 * the reference wherever the two names lie in the file (src/slimm.hpp:204-211 merges through a hash map).  Only a record
 * whose name was SHORTENED (no mate flag, ends in ".1" / ".2") can join records of another QNAME, and a run of adjacent
 * records with one canonical base is complete iff it holds an un-shortened record (the QNAME = base records are
 * contiguous, so they are these).  The library's decoders (slimm_push_bam_bytes, _bgzf_blocks, _sam_bytes) therefore count,
 * per file, the runs that consist of shortened names only; when there is one, slimm_analyze_alignments of the GROUPED
 * context returns SLIMM_E_REGROUP: the caller pushes the file again to a context created with SLIMM_ORDER_ANY, which is
 * exact whatever the order (the slimm command does that by itself).  A file without such names pays two register adds per
 * record.  A producer of decoded GROUPED records (slimm_push_records*, slimm_group_push_records*) applies the same rule with
 * slimm_host_q18_note / slimm_host_q18_regroup_needed below -- the library never sees its names.
 *
 * DECLARING A STREAM GROUPED IS A PROMISE THE LIBRARY DOES NOT CHECK BY ITSELF.  With record_order = SLIMM_ORDER_GROUPED
 * the front end compares adjacent records only: a read name that comes back after other names have been in between
 * becomes TWO reads (two unique reads where the reference, which merges through its hash map -- src/slimm.hpp:204-211 --
 * sees one multi-mapped read).  No error is raised, the profile is simply not the reference's.  Declare GROUPED only
 * what is grouped by construction (mapper output; @HD SO:queryname / GO:query, which is all the slimm command trusts);
 * everything else is SLIMM_ORDER_ANY.  slimm_check_grouping() is the diagnostic for a caller in doubt: after the
 * records are pushed it counts, on the device, the qName runs whose identity started an earlier run as well (0 = the
 * stream is grouped).  It costs a hash-set insert per run -- the set is a power of two of 8-byte entries at or above
 * twice the number of records: 16 to 32 bytes of device memory per record, up to 32 GiB near 2^31 records -- and is
 * therefore never run unasked; the slimm command runs it with --verify-grouping and warns.  Packed records are
 * compared by the 61 identity bits they carry (the four-array form: 62). */
int slimm_check_grouping(slimm_ctx* ctx, uint64_t* n_split_names);
int slimm_reserve(slimm_ctx* ctx, uint64_t n_records);
/* Append a batch from host memory (copied to the device before return). */
int slimm_push_records(slimm_ctx* ctx, const uint64_t* read_key, const int32_t* ref_id, const int32_t* begin_pos,
                       const uint16_t* flag, uint64_t n);
/* The same with a CHECK WORD per record: a second, independent hash of the read name (any 32 bits that equal names
 * share).  The library never sees names; with check words it can tell when two different names were given one key:
 * records with one key and different check words that meet -- next to each other in a GROUPED stream, after the device
 * sort for ANY order -- make slimm_finish_coverage return SLIMM_E_KEY_COLLISION instead of silently becoming one read
 * (the reference keys on the full name, src/slimm.hpp:204-211).  4 more bytes per record on the way in (and through
 * the sort).  Checked and unchecked pushes do not mix within a file. */
int slimm_push_records_checked(slimm_ctx* ctx, const uint64_t* read_key, const int32_t* ref_id, const int32_t* begin_pos,
                               const uint16_t* flag, const uint32_t* check, uint64_t n);
/* The lean form of the same stream: 16 bytes per record.  Of `flag` the record loop reads three bits -- unmapped
 * (src/slimm.hpp:197) and first / last in pair (src/slimm.hpp:205-208) -- and they ride in the key's top three bits:
 *   packed_key = (read_key & (2^61 - 1)) | mate << 61 | unmapped << 63,   mate = 1 (flag & 0x40), 2 (flag & 0x80), else 0
 * (slimm_pack_key / slimm_pack_keys do it; the identity of a qName is then its low 61 bits).  No flag array crosses the
 * bus or is read by the front end: 11 % fewer bytes on both.  Packed, unpacked and checked pushes do not mix within a
 * file.  slimm_push_records_packed_async is the streamed form (as slimm_push_records_async: the arrays must stay
 * unchanged until slimm_push_wait), slimm_set_records_device_packed the borrowed-device-arrays form. */
uint64_t slimm_pack_key(uint64_t read_key, uint16_t flag);
void slimm_pack_keys(const uint64_t* read_key, const uint16_t* flag, uint64_t n, uint64_t* packed_key);
int slimm_push_records_packed(slimm_ctx* ctx, const uint64_t* packed_key, const int32_t* ref_id, const int32_t* begin_pos,
                              uint64_t n);
int slimm_push_records_packed_async(slimm_ctx* ctx, const uint64_t* packed_key, const int32_t* ref_id,
                                    const int32_t* begin_pos, uint64_t n);
int slimm_set_records_device_packed(slimm_ctx* ctx, const uint64_t* d_packed_key, const int32_t* d_ref_id,
                                    const int32_t* d_begin_pos, uint64_t n);
/* RUN-MARKED records, 8 bytes each, for input grouped by read name (record_order = SLIMM_ORDER_GROUPED; anything else is
 * refused).  With the records of a name adjacent, the read identity the reference keys its hash map with (src/slimm.hpp:
 * 204-211) is "the qName run this record lies in" -- the device needs no name, only where a run starts.  A record is
 *   word      = reference id + 1 (0: not mapped -- the unmapped flag, src/slimm.hpp:197, or reference -1)
 *               | mate number << 29 (0 / 1 / 2, src/slimm.hpp:205-208) | (this record's qName differs from the one
 *               before it, or it is the file's first) << 31
 *   begin_pos
 * and the producer compares adjacent names instead of hashing them.  slimm_mark_word builds one word, slimm_mark_words
 * a batch from the four-array form (run starts where adjacent keys differ; *prev_key = the key in front of the batch,
 * NULL at the start of a file).  Half the bytes of the packed form cross the bus and are read by the front end.  What the
 * form gives up: there are no names to check -- slimm_check_grouping and the *_checked pushes do not apply -- and a file
 * is this form throughout.  _async / set_records_device / staged: as for the packed form (a staging set's ref_id array
 * holds the words). */
uint32_t slimm_mark_word(int32_t ref_id, uint16_t flag, int starts_run);
void slimm_mark_words(const uint64_t* read_key, const uint16_t* flag, const int32_t* ref_id, uint64_t n, const uint64_t* prev_key,
                      uint32_t* word);
int slimm_push_records_marked(slimm_ctx* ctx, const uint32_t* word, const int32_t* begin_pos, uint64_t n);
int slimm_push_records_marked_async(slimm_ctx* ctx, const uint32_t* word, const int32_t* begin_pos, uint64_t n);
int slimm_set_records_device_marked(slimm_ctx* ctx, const uint32_t* d_word, const int32_t* d_begin_pos, uint64_t n);
/* Streamed ingest.  slimm_push_records_async enqueues the copies on the context's copy stream and returns at once:
 * the arrays must stay unchanged until slimm_push_wait() returns (page-locked arrays are read by the DMA engine
 * directly; pageable ones still work, at the speed of the runtime's own staging).  slimm_analyze_alignments() is
 * ordered behind the copies on the device (an event), so the host never waits for PCIe: it decodes the next batch, or
 * drives another context's phases, meanwhile. */
int slimm_push_records_async(slimm_ctx* ctx, const uint64_t* read_key, const int32_t* ref_id, const int32_t* begin_pos,
                             const uint16_t* flag, uint64_t n);
int slimm_push_wait(slimm_ctx* ctx);
/* Two page-locked staging sets owned by the context, for producers that decode records piecemeal (the BAM reader of
 * the slimm command): fill set `which` (0 or 1; at least `capacity` records each), hand it over with
 * slimm_push_staged_async(ctx, which, n) and fill the other one meanwhile; slimm_staging_buffers / slimm_staging_wait
 * block until the set's last copy has left it. */
int slimm_staging_buffers(slimm_ctx* ctx, uint32_t which, uint64_t capacity, uint64_t** read_key, int32_t** ref_id,
                          int32_t** begin_pos, uint16_t** flag);
int slimm_push_staged_async(slimm_ctx* ctx, uint32_t which, uint64_t n);
/* The same for a set whose key array the producer filled with PACKED keys (slimm_pack_key; the set's flag array is not
 * read): 16 bytes per record over the bus. */
int slimm_push_staged_packed_async(slimm_ctx* ctx, uint32_t which, uint64_t n);
/* ... and for a set whose ref_id array holds run-marked words (slimm_mark_word; key and flag arrays are not read). */
int slimm_push_staged_marked_async(slimm_ctx* ctx, uint32_t which, uint64_t n);
int slimm_staging_wait(slimm_ctx* ctx, uint32_t which);
/* BAM ALIGNMENT RECORDS DECODED ON THE DEVICE.  Instead of decoding records on the host, a caller that holds a BAM file
 * inflates its BGZF blocks and hands over the bytes BEHIND the BAM header -- the alignment records as the SAM/BAM
 * specification lays them out (section 4.2: block_size | refID | pos | l_read_name | mapq | bin | n_cigar_op | flag | l_seq |
 * next_refID | next_pos | tlen | read_name | ...) -- in windows of any size, in file order; records may straddle windows.
 * The device finds the record boundaries and extracts what the record loop reads (src/slimm.hpp:194-208: refID, position,
 * flag, read name), appending to the context's record stream in the form its record order takes: SLIMM_ORDER_GROUPED ->
 * run-marked 8-byte records (a record starts a run where its NAME differs from the name of the record before it: exact,
 * no hash involved); SLIMM_ORDER_ANY -> key (the 62-bit hash of the name that host/alignment_file.cpp computes), refID,
 * position, flag and a check word (as slimm_push_records_checked).  `bytes`: any host memory (page-locked -- see
 * slimm_pin_host_buffer -- the DMA engine reads it directly).  A window's copy is started by the call that hands it
 * over and runs beside the device's work on the window BEFORE it: the buffer must stay unchanged until the NEXT call on
 * this context returns (a call with last != 0 finishes everything), so hand over three or more buffers in rotation.
 * *n_records (may be NULL): records appended by this call -- those of the windows it finished: a window is found, counted and
 * decoded once two later ones have been handed over or more than 4 GB of windows are in flight (they are copied, or inflated, meanwhile), all of them with last != 0.  last != 0: nothing follows (n_bytes may be 0) -- bytes of an incomplete record are then
 * an error (SLIMM_E_INVALID, "truncated BAM record"), as is a malformed record in any window.  A record longer than
 * 16 MiB is not supported in this form (SLIMM_E_INVALID: decode such a file on the host).  The forms do not mix within
 * a file.  Replaces: seqan::readRecord in src/slimm.hpp:194-208 / src/misc.hpp:509-522. */
int slimm_push_bam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, int last, uint64_t* n_records);
/* The same with the inflate on the device as well: `blocks` = n_bytes of whole BGZF blocks of the file (compressed, as they
 * lie in it, one behind the other, in file order across calls), of whose inflated bytes the first `skip` are not alignment
 * records (the BAM header, of any size, up to its end in the file's first record-bearing block; 0 in every later call).  The
 * compressed bytes cross the bus and are inflated on the device (slimm_amd/csrc/bgzf_tokens.hip: Huffman decode a lane per
 * block, matches filled a workgroup per block; bgzf_inflate.hip behind it; ISIZE, the DEFLATE blocks' form and the CRC32 are
 * checked), and the records are found and decoded as above.  Calls of any size: the library gathers them into device windows
 * of 1.4 - 1.9 GB of inflated bytes (tens of thousands of blocks) and inflates those on two streams in turn.  Windows of this
 * form and of slimm_push_bam_bytes may alternate within a file; buffer lifetime, `last`, *n_records and the errors are those of
 * slimm_push_bam_bytes, plus
 * SLIMM_E_INVALID for anything that is not a BGZF block or does not inflate to its ISIZE. */
int slimm_push_bgzf_blocks(slimm_ctx* ctx, const uint8_t* blocks, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* DEVICE MEMORY OF THE WINDOW PIPELINE.  A gathered window holds [16 MiB | up to 1.9 GB inflated] + its compressed bytes
 * (window / ratio + one push) + 16 B per block + the inflater's scratch (~0.36 B per inflated byte, two sets) + 456 record
 * offsets per 16 KB; up to four windows are in turn in flight.  slimm_set_input_size_hint(ctx, the file's COMPRESSED size),
 * called before a file's first window, lets the library reserve exactly what the file will use at its first push (a 70 MB
 * file: one window of ~0.3 GB; a file of many gigabytes: four windows, ~14 GB at a ratio of 3) -- reserving ahead matters
 * because an allocation made while inflate kernels run waits for them.  Without a hint nothing is reserved ahead and buffers
 * appear as windows need them (the same totals, some stalls).  slimm_reset keeps up to 4 GiB of these buffers for the next
 * file and releases them above that; slimm_window_memory reports what is held.  The hint is per file (cleared by slimm_reset).
 * bzip2 SAM (slimm_push_bzip2_sam_bytes) gathers no compressed window on the device: a batch of blocks is decoded at a time,
 * with 4.5 MB of scratch per block of the batch (900 kB of BWT string -- then its RLE1 text -- and 3.6 MB of inverse-BWT
 * links) + 1 KB of byte histogram, for 16 to 256 blocks (the hint / 64 kB; 64 without a hint): at most 1.15 GB, sized for
 * each file at its first decode (it grows, never shrinks, between files; slimm_reset releases it with the rest above 4 GiB);
 * plus the compressed bytes of a round (the pushes since the last one, at most 448 MB reserved from the hint) and 8 B per
 * block magic found.  Its text windows take the ring of window buffers above, one batch's text
 * each (< 1.9 GB): within today's total of <= 17 GB per file.
 * gzip SAM (slimm_push_gzip_sam_bytes) sizes nothing before the size pass has counted a round's text: the compressed bytes
 * of a round (the pushes since the last one), 8 B per block candidate and 24 B per chunk start, then per round 2 B per byte
 * of text (the symbols: at most 512 MB of text a round, or one chunk alone of up to 1 GiB), 32 KiB + 72 B per chunk of the
 * chain and 8 B per 2 KiB of text.  A round of more text is split at a chunk boundary; a single deflate block of more than
 * 1 GiB of text is refused.  slimm_window_memory counts all of it.
 * zstd SAM (slimm_push_zstd_sam_bytes) sizes everything from the block headers and, for the text, from the decoded
 * sequences: the compressed bytes of a round, 120 B per block, the Huffman-coded literals' bytes, 12 B per sequence, and per
 * byte of a round's text (at most 512 MB by the blocks' bounds) 1 B + 4 B for the position it copies from, plus twice the
 * frame's window (at most 128 MiB) of history; a frame that states a checksum also takes a page-locked host copy of the
 * round's text, which is host memory (slimm_window_memory does not count it) and is released by slimm_reset.
 * xz SAM (slimm_push_xz_sam_bytes) sizes everything from the chunk headers, which state every size: the compressed bytes of
 * a round, 1 B per byte of its text (at most 512 MB, or one block alone of up to 1 GiB; the text is the blocks' dictionary
 * as well: no 16-bit symbols, no history), 104 B per block and 16 B per 2 KiB of text.  slimm_window_memory counts all of it.
 * lzip SAM (slimm_push_lzip_sam_bytes) sizes everything from the members' trailers in the same way: the compressed bytes of a
 * round, 1 B per byte of its text, 104 B per member and 16 B per 2 KiB of text. */
int slimm_set_input_size_hint(slimm_ctx* ctx, uint64_t compressed_bytes);
int slimm_window_memory(slimm_ctx* ctx, uint64_t* device_bytes);
/* hipMemGetInfo of the context's device: bytes in use (by every process and context on it) and the device's total. */
int slimm_device_memory(slimm_ctx* ctx, uint64_t* used_bytes, uint64_t* total_bytes);
/* SAM TEXT decoded on the device (slimm_amd/csrc/sam_decode.hip): the reference takes .sam and .bam alike
 * (src/file_helper.hpp:73-75; the record loop src/slimm.hpp:194-208 reads QNAME, FLAG, RNAME -> reference index, POS).
 * `text` = the file's alignment lines, everything behind the header, in windows cut ANYWHERE (the incomplete last line of a
 * window is carried in front of the next one; a last line without its newline is a line); same buffer-lifetime and window
 * rules as slimm_push_bam_bytes, the two do not mix within a file.  RNAME is looked up in the header's reference names, which
 * slimm_set_reference_names(ctx, names[n_refs]) hands over once per context (index = reference id; "*" and names the header
 * does not have give no reference, like the host reader); QNAME is compared with the line before (grouped input) or hashed
 * (any order) in its canonical form (quirk Q18).  A line with fewer than ten fields is an error like the host reader's; a
 * header line or an empty line AMONG the alignment lines (which the host reader skips) is refused with "decode this file on
 * the host". */
int slimm_set_reference_names(slimm_ctx* ctx, const char* const* names);
int slimm_push_sam_bytes(slimm_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int last, uint64_t* n_records);
/* BGZF-COMPRESSED SAM TEXT (`bgzip x.sam`) with the inflate on the device as well: `blocks` = n_bytes of whole BGZF blocks
 * of the file, in file order across calls, of whose inflated bytes the first `skip` are the header (in front of the first
 * alignment line; 0 in every later call).  The blocks are gathered, inflated and checked as by slimm_push_bgzf_blocks, and
 * the inflated text is found and decoded as by slimm_push_sam_bytes (slimm_set_reference_names first); a line straddles
 * windows as there.  Windows of this form and of slimm_push_sam_bytes (text the caller inflated) may alternate within a file;
 * SAM and BAM do not mix.  A file's last line without its newline is a line also when the device inflated it (the caller
 * never sees those bytes).  Errors: those of the two, SLIMM_E_INVALID "corrupt BGZF block" among them. */
int slimm_push_bgzf_sam_blocks(slimm_ctx* ctx, const uint8_t* blocks, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* BZIP2-COMPRESSED SAM TEXT (`bzip2 x.sam`; pbzip2 / lbzip2: streams back to back, of any levels) decoded on the device:
 * `bytes` = the file's next n_bytes, from its first byte on and in order across calls, cut anywhere (inside a block, inside
 * a magic); of the decoded text the first `skip` bytes are the header (in front of the first alignment line; 0 in every
 * later call).  Pushes are gathered on the host and decoded in rounds: the device finds block magics at every bit offset,
 * decodes the blocks of a batch at once (Huffman, MTF, inverse BWT, RLE1), checks every block CRC and -- on the host --
 * each stream's combined CRC, and hands the text to the SAM finder and decoder as slimm_push_sam_bytes does
 * (slimm_set_reference_names first).  The caller's buffer is free when the call returns.  A block whose bytes have not all
 * come yet waits for the next push.  This form does not mix with the others within a file.  Errors: SLIMM_E_INVALID
 * "bzip2-compressed input is not supported unless it decodes: <where>: <cause>" -- truncation, a bad Huffman code, a block
 * or combined CRC mismatch, origPtr out of range, a block longer than its level allows, a randomised block (never
 * written since bzip2 0.9.5: refused), bytes after the last end-of-stream marker. */
int slimm_push_bzip2_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* GZIP-COMPRESSED SAM TEXT (`gzip x.sam`: one member, or members back to back, empty ones among them; FEXTRA, FNAME,
 * FCOMMENT and FHCRC in any member header) inflated on the device (slimm_amd/csrc/gzip_decode.hip).  The contract is that of
 * slimm_push_bzip2_sam_bytes: `bytes` = the file's next n_bytes, from its first byte on and in order across calls, cut
 * anywhere (inside a member header, a block, a trailer); of the inflated text the first `skip` bytes are the header (0 in
 * every later call); slimm_set_reference_names first; the caller's buffer is free when the call returns; what cannot be
 * decoded yet waits for the next push; the form does not mix with the others within a file.  Pushes are gathered on the
 * host and decoded in rounds: the device finds the headers of non-final dynamic blocks at every bit offset (candidates, none
 * of them trusted), decodes chunks of the stream from the chosen ones in parallel -- first for their sizes, then for their
 * text, with markers where a copy reaches in front of the chunk --, keeps of each only what the chain from the member's first
 * block confirms, resolves the markers from the chunk in front, and checks every member's CRC32 and ISIZE.  A BGZF file is a
 * gzip file too; callers tell it apart beforehand and give it to slimm_push_bgzf_sam_blocks.  Errors: SLIMM_E_INVALID
 * "truncated gzip stream" (also for a cut inside the trailer) and "corrupt gzip stream (<cause>)" -- a bad code, an
 * over-subscribed or incomplete code set, a distance beyond the member's start, a stored block whose LEN and NLEN disagree,
 * a CRC32 or ISIZE mismatch, bytes behind the last member that start no member -- in the words of the host reader. */
int slimm_push_gzip_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* The counters of the gzip file read last (they outlive slimm_reset, and are zeroed by the next gzip file's first push):
 * out[0] members, [1] chunks decoded on the chain, [2] candidates found, [3] candidates and chunk starts dropped by the chain,
 * [4] stored, [5] fixed and [6] dynamic deflate blocks, [7] back-reference bytes resolved from the window of the chunk in
 * front, [8] rounds, [9] bytes of text, [10] compressed bytes, [11] chunk starts added by SLIMM_FORCE gzip_false_starts. */
int slimm_get_gzip_stats(slimm_ctx* ctx, uint64_t out[12]);
/* ZSTD-COMPRESSED SAM TEXT (`zstd x.sam`; pzstd / cat: frames back to back; skippable frames among them are passed over)
 * decoded on the device (slimm_amd/csrc/zstd_decode.hip; the format: zstd_frame.h).  The contract is that of
 * slimm_push_gzip_sam_bytes: `bytes` = the file's next n_bytes, from its first byte on and in order across calls, cut
 * anywhere (inside a frame header, a block header, a block, the checksum); of the decoded text the first `skip` bytes are the
 * header (0 in every later call); slimm_set_reference_names first; the caller's buffer is free when the call returns; what
 * cannot be decoded yet waits for the next push; the form does not mix with the others within a file.  Behind
 * slimm_set_input_mid_file it is a byte range of a split file, taken only when slimm_set_input_range has told where the
 * range lies (below: "zstd SAM by byte range"); without that it is refused ("a zstd stream is not cut by byte range unless
 * its range is announced (slimm_set_input_range) and starts at a frame").  Pushes are gathered on the host and decoded
 * in rounds (32 MiB of compressed bytes, at most 512 MB of text by the blocks' bounds): the host walks the frame and block
 * headers, the device decodes every compressed block's literals and sequences at once (a wave per block), builds the
 * round's text in parallel over its bytes -- a match byte gets the position it copies from, in the round or in the
 * frame's last window of text kept from the round before; pointer doubling resolves the chains -- and the host checks the
 * content size and the content checksum (XXH64) of a frame that states them.  Limits: a window of more than 128 MiB is
 * refused (as `zstd -d` does without --long), so is a dictionary id other than 0.  Errors: SLIMM_E_INVALID "zstd-compressed
 * input is not supported unless it decodes: <where>: <cause>" in the words of the host reader -- truncation (also inside
 * the checksum), a reserved bit or block type, bad Huffman weights, a bad FSE table description, a bitstream that does not
 * end on its padding bit, a block larger than its maximum, a literals or sequence total that disagrees with the block, an
 * offset beyond the frame's start or window, a content size or checksum mismatch, bytes behind the last frame that start
 * no frame. */
int slimm_push_zstd_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* The counters of the zstd file read last (they outlive slimm_reset, and are zeroed by the next zstd file's first push):
 * out[0] frames, [1] skippable frames, [2] raw, [3] RLE and [4] compressed blocks, literals sections [5] Huffman-coded with
 * a tree, [6] treeless, [7] raw or RLE, sequence tables [8] predefined, [9] of one symbol (RLE), [10] FSE-described,
 * [11] repeated, [12] sequences, [13] match bytes copied from in front of their own block, of which [14] from the history
 * of an earlier round, [15] rounds, [16] bytes of text, [17] compressed bytes, [18] content checksums checked, [19] the most
 * pointer-doubling passes a round took (at most ceil(log2(its text + history)) + 1). */
int slimm_get_zstd_stats(slimm_ctx* ctx, uint64_t out[20]);
/* LZ4-COMPRESSED SAM TEXT (`lz4 x.sam`, `lz4 -BD`: linked blocks; frames back to back; skippable frames among them are passed
 * over) decoded on the device (slimm_amd/csrc/lz4_decode.hip; the format: lz4_frame.h, the container: lz4_walk.h).  The
 * contract is that of slimm_push_zstd_sam_bytes: `bytes` = the file's next n_bytes, from its first byte on and in order
 * across calls, cut anywhere (inside a frame header, a block header, a block, a checksum); of the decoded text the first
 * `skip` bytes are the header (0 in every later call); slimm_set_reference_names first; the caller's buffer is free when the
 * call returns; what cannot be decoded yet waits for the next push; the form does not mix with the others within a file.
 * Behind slimm_set_input_mid_file it is refused: "an lz4 stream is not cut by byte range".  Pushes are gathered on the host
 * and decoded in rounds (32 MiB of compressed bytes, at most 512 MB of text by the blocks' bounds; SLIMM_FORCE lz4_round=N,
 * lz4_round_text=N): the host walks the frame and block headers and checks the header and block checksums (XXH32), the
 * device walks every compressed block's tokens at once (a wave per block, the bytes staged through LDS), builds the round's
 * text in parallel over its bytes -- a literal byte is read from the block, a match byte gets the position it copies from,
 * in the round or in a linked frame's last 64 KiB of text kept from the round before; pointer doubling resolves the chains
 * -- and the host checks the content size and the content checksum (XXH32) of a frame that states them.  Limits: a
 * dictionary id and the legacy format (`lz4 -l`) are refused.  Errors: SLIMM_E_INVALID "lz4-compressed input is not
 * supported unless it decodes: <where>: <cause>" in the words of the host reader -- truncation, a version other than 1, a
 * reserved bit, a block larger than its maximum, a header, block or content checksum mismatch, a content size mismatch, an
 * offset of 0 or beyond the frame's start (in an independent frame: the block's), a block that ends inside a length, its
 * literals or an offset, or behind a match, bytes behind the last frame that start no frame. */
int slimm_push_lz4_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* The counters of the lz4 file read last (they outlive slimm_reset, and are zeroed by the next lz4 file's first push):
 * out[0] frames, [1] skippable frames, [2] linked frames, [3] stored and [4] compressed blocks, [5] sequences (matches),
 * [6] match bytes copied from in front of their own block, of which [7] from the history of an earlier round, [8] rounds,
 * [9] bytes of text, [10] compressed bytes, [11] block checksums and [12] content checksums checked, [13] the most
 * pointer-doubling passes a round took (at most ceil(log2(its text + history)) + 1); [14], [15]: 0. */
int slimm_get_lz4_stats(slimm_ctx* ctx, uint64_t out[16]);
/* XZ-COMPRESSED SAM TEXT (`xz x.sam`; xz -T, --block-size, pixz, pxz: many blocks; streams back to back with stream padding)
 * decoded on the device (slimm_amd/csrc/xz_decode.hip; the format: xz_stream.h).  The contract is that of
 * slimm_push_zstd_sam_bytes: `bytes` = the file's next n_bytes, from its first byte on and in order across calls, cut
 * anywhere (inside a stream header, a block header, a chunk header, a chunk, the check, the index, the footer); of the decoded
 * text the first `skip` bytes are the header (0 in every later call); slimm_set_reference_names first; the caller's buffer
 * is free when the call returns; what cannot be decoded yet -- a block whose bytes have not all come -- waits for the next
 * push; the form does not mix with the others within a file.  Behind slimm_set_input_mid_file it is a byte range of a split
 * file, taken only when slimm_set_input_range has told where the range lies ("xz SAM by byte range" below; otherwise "an xz
 * stream is not cut by byte range unless its range is announced (slimm_set_input_range) and starts at a block").  Pushes are gathered on the host and decoded in rounds (32 MiB of compressed bytes; the whole
 * blocks at hand, at most 512 MB of text or one block alone): the host reads stream headers, block headers, indexes and
 * footers and walks every block's LZMA2 chunk headers, which state all sizes; the device decodes the blocks, ONE LANE PER
 * BLOCK, each into its place in the round's text, computes every block's CRC32 or CRC64 from pieces, and the host compares
 * them with the check fields and every index with the blocks in front of it.  A file of few blocks therefore keeps few
 * lanes busy: the library decodes whatever it is pushed, the `slimm` command reads such a file on the host.  Limits: LZMA2 is
 * the one filter (BCJ and delta chains are refused, the filter named); a block of more than 1 GiB of text is refused
 * ("decode this file on the host"); SHA-256 checks are NOT verified (the blocks are counted: out[10] below); check kinds
 * other than none, CRC32, CRC64 and SHA-256 are refused.  Errors: SLIMM_E_INVALID "xz-compressed input is not supported
 * unless it decodes: <where>: <cause>" in the words of the host reader -- truncation, a header, index or footer CRC32
 * mismatch, reserved flags, a bad block header or dictionary size, a bad control byte, a first chunk that does not reset the
 * dictionary, an LZMA chunk without properties or (behind an uncompressed chunk) without a state reset, lc + lp > 4, a
 * distance beyond the block's start or dictionary, a match that runs over its chunk's end, a chunk that does not end where
 * its compressed size says, a range coder that does not end at zero, sizes that disagree with the block header, bad
 * padding, "check mismatch", "index does not match the blocks", bytes behind the last stream that are neither padding nor
 * a stream. */
int slimm_push_xz_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* The counters of the xz file read last (they outlive slimm_reset, and are zeroed by the next xz file's first push):
 * out[0] streams, [1] blocks, [2] LZMA chunks, [3] uncompressed chunks, [4] LZMA chunks that reset the state, [5] ... that set
 * a properties byte, [6] ... other than the default 0x5D (lc 3, lp 0, pb 2), blocks by check kind: [7] none, [8] CRC32,
 * [9] CRC64, [10] SHA-256 (not verified), [11] match bytes, [12] the longest distance, [13] rounds, [14] bytes of text,
 * [15] compressed bytes, [16] index records checked against their blocks. */
int slimm_get_xz_stats(slimm_ctx* ctx, uint64_t out[17]);
/* LZIP-COMPRESSED SAM TEXT (`lzip x.sam`, `plzip x.sam`: many members back to back) decoded on the device
 * (slimm_amd/csrc/lzip_decode.hip; the format: lzip_member.h, the member finder: lzip_walk.h).  The contract is that of
 * slimm_push_xz_sam_bytes: `bytes` = the file's next n_bytes, from its first byte on and in order across calls, cut anywhere
 * (inside a header, a stream, a trailer); of the decoded text the first `skip` bytes are the header (0 in every later call);
 * slimm_set_reference_names first; the caller's buffer is free when the call returns; what cannot be decoded yet -- a member
 * whose end has not come -- waits for the next push; the form does not mix with the others within a file.  Behind
 * slimm_set_input_mid_file it is refused ("an lzip stream is not cut by byte range").  A member's sizes lie in its trailer,
 * so the host FINDS a member's end: the offset q at which the next legal header (or, at the last push, the end of the bytes)
 * stands and the eight bytes in front of q say q minus the member's start; a magic inside compressed data fails that test
 * and is passed over; what has been searched is not searched again.  Pushes are gathered on the host and decoded in rounds
 * (32 MiB of compressed bytes; the whole members at hand, at most 512 MB of text or one member alone; SLIMM_FORCE
 * lzip_round=N, lzip_round_text=N): the device decodes the members, ONE LANE PER MEMBER, each into its place in the round's
 * text, which is its dictionary; computes every member's CRC32 from pieces; the host compares them with the trailers.  A
 * file of few members therefore keeps few lanes busy: the library decodes whatever it is pushed, the `slimm` command reads
 * such a file on the host.  Memory: the compressed bytes of a round, 1 B per byte of its text, 104 B per member and 16 B per
 * 2 KiB of text; slimm_window_memory counts all of it.  Limits: a member of more than 1 GiB of text is refused ("decode this
 * file on the host"); version 0 members and the legacy `.lzma` format are not read.  Errors: SLIMM_E_INVALID
 * "lzip-compressed input is not supported unless it decodes: <where>: <cause>" in the words of the host reader --
 * truncation, "trailing data behind the last lzip member", a version other than 1, a dictionary size below 4 KiB or above
 * 512 MiB, a range coder that does not start with a zero byte or end at zero, a distance beyond the member's start or
 * dictionary, a match that runs over the member's data_size, an end marker in front of it, text that goes on behind it, a
 * sync-flush marker, an end marker of a length other than 2, a stream that does not end at the trailer, "CRC32 mismatch". */
int slimm_push_lzip_sam_bytes(slimm_ctx* ctx, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records);
/* The counters of the lzip file read last (they outlive slimm_reset, and are zeroed by the next lzip file's first push):
 * out[0] members, [1] of them empty (no text), [2] rounds, [3] CRC32 fields checked, [4] match bytes, [5] the longest
 * distance, [6] the largest dictionary size a header stated, [7] bytes of text, [8] compressed bytes. */
int slimm_get_lzip_stats(slimm_ctx* ctx, uint64_t out[9]);
/* The members of a regular lzip file by its trailers alone: from the file's end, a trailer's member_size names its member's
 * first byte, in front of which the trailer of the member before lies; every header is held against the format.  A few
 * reads, nothing decoded.  *n_members and the sum of the stated data_sizes; SLIMM_E_INVALID when the chain does not close
 * on byte 0 (trailing data, a truncated file, not an lzip file). */
int slimm_host_lzip_members(const char* path, uint64_t* n_members, uint64_t* text_bytes);
/* Page-locks a buffer of the caller (hipHostRegister) until the context is destroyed: copies out of it then run at the
 * speed of the bus instead of the runtime's own staging. */
int slimm_pin_host_buffer(slimm_ctx* ctx, const void* buffer, uint64_t n_bytes);
/* Use records already resident in device memory, without copying; the arrays must stay valid and unchanged
 * until slimm_reset().  Replaces anything pushed before. */
int slimm_set_records_device(slimm_ctx* ctx, const uint64_t* d_read_key, const int32_t* d_ref_id,
                             const int32_t* d_begin_pos, const uint16_t* d_flag, uint64_t n);
/* The device arrays of the records a context holds after its pushes, whatever brought them there (decoded records, or the
 * window pipeline's decoders): for a caller that hands stretches of them to other contexts (slimm_set_records_device*) -- a
 * group that lets ONE member read and decode a file does (slimm_group_get_profiles).  *form: 0 four arrays, 1 packed
 * (d_flag NULL), 2 run-marked (d_read_key and d_flag NULL, d_ref_id holds the words).  Waits for the context's copies and
 * decode kernels; the pointers stay valid until slimm_reset / slimm_destroy. */
int slimm_records_device(slimm_ctx* ctx, const uint64_t** d_read_key, const int32_t** d_ref_id, const int32_t** d_begin_pos,
                         const uint16_t** d_flag, uint64_t* n, int* form);

/* ---- phase A: slimm::analyze_alignments() (src/slimm.hpp:191-303) on this context's records:
 * grouping by read, first-bin per (read, ref), cov / uniq_cov histograms.  Local to this GPU. */
int slimm_analyze_alignments(slimm_ctx* ctx);

/* Stream-ordered exchange.  The context's kernels run on one HIP stream (slimm_get_stream: a hipStream_t).  By default
 * every function that hands out a device buffer for a collective synchronises that stream first, so that any stream
 * may read the buffer.  A caller that enqueues its collectives ON the context's stream (ncclAllGather(..., stream),
 * torch.cuda.ExternalStream) turns that off with slimm_set_stream_ordered(ctx, 1): buffers are then valid in stream
 * order only, and between slimm_analyze_alignments and the cut-offs the host never waits for the device. */
int slimm_get_stream(slimm_ctx* ctx, void** hip_stream);
int slimm_set_stream_ordered(slimm_ctx* ctx, int on);

/* Multi-GPU exchange point (no reference counterpart; reads are sharded across ranks):
 * device buffer [cov | uniq_cov | 16 scalar words] of *n_words uint32 that the caller sums across ranks in place
 * (one all-reduce) between slimm_analyze_alignments() and slimm_finish_coverage().  The stream is synchronised. */
int slimm_coverage_buffer(slimm_ctx* ctx, void** d_ptr, uint64_t* n_words);
/* The third coverage array, uniq_cov2 (reference_contig.hpp:112), after slimm_filter_alignments / slimm_install_merged_
 * partials: *n_words uint32 (every reference padded like in slimm_coverage_buffer) that the caller may sum across ranks
 * in place so that slimm_get_bins(ctx, 2, ...) returns the global array.  The stream is synchronised unless
 * slimm_set_stream_ordered is on. */
int slimm_uniq_cov2_buffer(slimm_ctx* ctx, void** d_ptr, uint64_t* n_words);

/* Multi-GPU, optional: announce before slimm_analyze_alignments that slimm_coverage_summary will be called, so that
 * the histogram kernels write the 'bin != 0' bitmaps while the finished tiles are still in LDS (otherwise
 * slimm_coverage_summary streams both coverage arrays once more to build them).  n_slices: 0 = off; 1 = one
 * [cov bits | uniq_cov bits] block (all-gather form, below); n > 1 = the bitmaps cut into n slices of bin tiles, slice j
 * = [cov bits | uniq_cov bits] of rank j's share, for the all-to-all form. */
int slimm_prepare_summary(slimm_ctx* ctx, uint32_t n_slices);

/* The coverage arrays (cov, uniq_cov, uniq_cov2: reference src/reference_contig.hpp:70-72) are intermediate results of
 * the path: the profile needs their per-reference sums and non-zero bin counts, which the tile kernels take from every
 * finished tile while it is in LDS.  on = 0 before slimm_analyze_alignments: the finished tiles are not written to HBM
 * (only what the reference's -co output, slimm_get_bins and slimm_coverage_buffer would read); those calls then fail
 * with SLIMM_E_INVALID.  Default: on = 1. */
int slimm_keep_bins(slimm_ctx* ctx, int on);
/* Leaner exchange for the same point, used by default by slimm_amd/distributed.py: the cut-offs only need per-reference
 * SUMS of cov / uniq_cov (additive) and per-reference counts of NON-ZERO bins (popcount of the OR of every rank's
 * "bin != 0" bitmap).  slimm_coverage_summary() builds [sums | 16 scalars | cov bits | uniq_cov bits] for this rank in
 * device memory (*n_words uint32, about 1/16 of the bins); the caller all-gathers the summaries of all ranks into one
 * device buffer (rank-major, contiguous) and hands it to slimm_finish_coverage_merged(), which replaces
 * slimm_finish_coverage().  cov / uniq_cov then stay per-rank partial sums (slimm_get_bins returns this rank's share).
 * Device memory the caller hands in (here and in the calls below) is read by kernels on the CONTEXT'S stream
 * (slimm_get_stream), which waits for no other stream: whatever wrote it -- a collective, a copy -- must be complete, or have
 * been enqueued on that stream. */
int slimm_coverage_summary(slimm_ctx* ctx, void** d_ptr, uint64_t* n_words);
int slimm_finish_coverage_merged(slimm_ctx* ctx, const void* d_gathered, uint32_t n_ranks);
/* All-to-all form of the same exchange for many ranks (each rank receives 1/n of every other rank's bitmaps instead of
 * all of them).  With slimm_prepare_summary(ctx, n) in effect the buffer of slimm_coverage_summary is
 * [4 n_refs + 16 words | n chunks of equal size]; send chunk j to rank j (ncclAllToAll / all_to_all_single) and hand the
 * n received chunks to slimm_merge_summary_slices: it ORs them, counts the non-zero bins of this rank's slice per
 * reference and returns a device vector of 4 n_refs + 16 words [own sums, partial non-zero counts | own scalars] that
 * the ranks sum in place (all-reduce, int32).  slimm_finish_coverage_reduced then takes the place of
 * slimm_finish_coverage. */
int slimm_merge_summary_slices(slimm_ctx* ctx, const void* d_received, uint32_t n_ranks, uint32_t my_rank, void** d_vec,
                               uint64_t* n_words);
int slimm_finish_coverage_reduced(slimm_ctx* ctx);

/* End of phase A: per-reference reads_count / uniq_reads_count / non-zero bin counts
 * (reference_contig.hpp:84-91,148-155) from the (reduced) bins, and the float statistics of src/slimm.hpp:259-302.
 * Returns SLIMM_E_NO_HITS when hits_count == 0. */
int slimm_finish_coverage(slimm_ctx* ctx);

/* Install phase-A per-reference results computed elsewhere, instead of slimm_analyze_alignments() +
 * slimm_finish_coverage(): for host-only contexts (device = -1, no GPU touched) that run just the scalar host part
 * of the path -- cut-offs, propagation, profile -- e.g. on a rank that merges results.  uniq_matches is the sum of
 * uniq_reads_count. */
int slimm_set_coverage_columns(slimm_ctx* ctx, const uint32_t* reads_count, const uint32_t* uniq_reads_count,
                               const uint32_t* nz_cov, const uint32_t* nz_uniq_cov, uint32_t hits_count,
                               uint32_t matches_count);

/* ---- phase B + C(1): slimm::filter_alignments() (src/slimm.hpp:351-392): cut-offs (coverage_cut_off :328-344,
 * uniq_coverage_cut_off :672-688, get_quantile_cut_off misc.hpp:197-216), valid set, per-read update
 * (read_stat.hpp:98-114), uniq_cov2 -- fused on the device with the per-read LCA of
 * get_reads_lca_count() step 1 (src/slimm.hpp:536-557, get_lca :516-531). Local to this GPU. */
int slimm_filter_alignments(slimm_ctx* ctx);

/* Multi-GPU form of slimm_filter_alignments with ONE host synchronisation for the whole phase: this call only
 * launches (the device work of slimm_filter_alignments plus the packing of this rank's additive partial results);
 * the caller sums the buffer of slimm_partials_buffer across ranks on the context's stream (slimm_get_stream) and
 * calls slimm_install_merged_partials, which copies the merged results to the host and synchronises.  When the
 * (taxon, reference) pair set of SOME rank overflowed (the flag travels with the sums, so every rank sees it),
 * slimm_install_merged_partials returns SLIMM_E_RETRY on every rank -- each has grown its table -- and the caller
 * goes round again: launch, sum, install. */
int slimm_filter_alignments_launch(slimm_ctx* ctx);

/* Multi-GPU: the additive partial results of phase B/C(1) of this rank, to be merged across ranks by the caller.
 *   uniq_reads_count2 [n_refs], lca_count [n_taxa_dense] (sum), level_marks [n_refs] (bitwise OR),
 *   pairs: (dense taxon << 32 | ref) of reads whose refs agree at no level (set union), scalars[4] (sum). */
typedef struct {
    uint32_t n_refs, n_taxa_dense;
    uint32_t* uniq_reads_count2;
    uint32_t* lca_count;
    uint32_t* level_marks;
    uint64_t* pairs;
    uint32_t n_pairs;
    uint32_t scalars[4]; /* [0] uniq_matches_count2 */
} slimm_partials;
/* The dense taxon index used by lca_count and pairs: ascending distinct taxids of the lineage table. */
int slimm_dense_taxa(slimm_ctx* ctx, uint32_t* n, const uint32_t** taxid);
int slimm_get_partials(slimm_ctx* ctx, slimm_partials* out);       /* pointers stay owned by ctx, valid until reset */
int slimm_set_partials(slimm_ctx* ctx, const slimm_partials* in);  /* install merged values (copied) */

/* Multi-GPU, device-side merge of the additive partial results (faster than get/set_partials through the host).
 * After slimm_filter_alignments: a device buffer of n_words 32-bit words
 *   [n_refs uniq_reads_count2 | n_taxa_dense LCA counts | 2 n_refs level marks, one 8-bit field per level | 1 pair count]
 * that the ranks sum in place (ncclAllReduce(ncclSum, ncclInt32) from C++, torch.distributed.all_reduce on a tensor
 * aliasing it); at most 255 ranks, so that no field carries into the next.  slimm_install_merged_partials then copies
 * it back and installs it.  *total_pairs = (taxon, reference) pairs over all ranks (src/slimm.hpp:551-556, the
 * no-level-agrees case): when it is not zero, gather every rank's pairs (slimm_get_partials) and install the union with
 * slimm_set_partials. */
int slimm_partials_buffer(slimm_ctx* ctx, void** d_ptr, uint64_t* n_words);
int slimm_install_merged_partials(slimm_ctx* ctx, uint32_t* total_pairs);

/* ---- phase C(2,3): the propagation part of slimm::get_reads_lca_count() (src/slimm.hpp:560-610). */
int slimm_get_reads_lca_count(slimm_ctx* ctx);

/* THE ORDER OF THE PROPAGATION (quirk Q17).  Step 2 (src/slimm.hpp:560-586) hands the read count and the children of every
 * directly counted taxon up the lineage of that taxon's smallest child AT THE MOMENT IT IS WALKED, and the reference walks
 * an unordered_map: where an earlier climb can hand a later taxon a smaller child of another lineage -- databases with
 * lineage holes, taxid 0 in a rank slot, once some multi-mapped read's LCA is taxid 0 -- the reference's own counts depend
 * on its hash table's bucket order and cannot be reproduced from the input.
 *   WHICH WALK THE LIBRARY TAKES: the directly counted taxa by rank, lowest (strain) first -- a taxid the database does
 * not name, taxid 0 among them, counts as a strain (Q6) --, and ascending taxid within a rank (SLIMM_WALK_DEFAULT);
 * SLIMM_WALK_REVERSED is its exact reverse.  slimm_set_propagation_priority puts the listed taxids that are directly
 * counted in front, in the listed order (ids that are unknown or not counted are ignored, a repeated id counts once; n = 0
 * clears the list); the rest follow in the chosen walk.  Both are settings of the context like its configuration: they
 * hold for every later slimm_get_reads_lca_count and survive slimm_reset.  For a group set them on
 * slimm_group_context(g, 0), the member that propagates, and read the verdict there.
 *   slimm_get_reads_lca_count also decides whether the walk matters for THIS file, over every walk and whichever was
 * taken; slimm_get_propagation_order reports it until the context's next propagation or reset (an error before any):
 *   SLIMM_PROPAGATION_INDEPENDENT  every order of the walk gives the same counts and the same children (proved);
 *   SLIMM_PROPAGATION_DEPENDENT    two concrete walks were run and their step-2 results differ;
 *   SLIMM_PROPAGATION_UNDECIDED    neither: not proved independent, and the walks tried (default, reversed, each taxon
 *                                  below -- at most 16 of them -- first and last) agree.
 * and for the last two the taxa involved, as taxids in ascending order: the directly counted taxa that can receive
 * children from another counted taxon's climb before their own walk when that can change the lineage they climb or where
 * those children travel.  taxid may be NULL to ask for the count (*n_taxa); otherwise cap entries are available. */
enum { SLIMM_PROPAGATION_INDEPENDENT = 0, SLIMM_PROPAGATION_DEPENDENT = 1, SLIMM_PROPAGATION_UNDECIDED = 2 };
enum { SLIMM_WALK_DEFAULT = 0, SLIMM_WALK_REVERSED = 1 };
int slimm_get_propagation_order(slimm_ctx* ctx, int* verdict, uint32_t* taxid, uint32_t cap, uint32_t* n_taxa);
int slimm_set_propagation_walk(slimm_ctx* ctx, int walk);
int slimm_set_propagation_priority(slimm_ctx* ctx, const uint32_t* taxid, uint32_t n);

/* The per-file body of slimm::get_profiles() (src/slimm.hpp:447-489) on one GPU in one call:
 * slimm_analyze_alignments, slimm_finish_coverage, slimm_filter_alignments, slimm_get_reads_lca_count and, when path is
 * not NULL, slimm_write_abundance_file.  Returns SLIMM_E_NO_HITS (nothing written) when no record is mapped. */
int slimm_get_profiles(slimm_ctx* ctx, const char* path);

/* ---- slimm::write_abundance() (src/slimm.hpp:733-843): the final profile.  The text is identical in format to
 * the reference's <prefix>_profile.tsv; rows come in ascending taxid order (the reference's order is that of an
 * unordered_map and carries no meaning).  The buffer is owned by ctx. */
int slimm_write_abundance(slimm_ctx* ctx, const char** text, uint64_t* len);
/* Same, written to a file (path = get_tsv_file_name(...) result, computed by the caller). */
int slimm_write_abundance_file(slimm_ctx* ctx, const char* path);

/* ---- results (the public members of class slimm, src/slimm.hpp:105-127) ---- */
typedef struct {
    uint32_t hits_count, matches_count, uniq_matches_count, uniq_hits_count, uniq_matches_count2;
    uint32_t reference_count, matched_ref_length;
    uint32_t failed_by_cov, failed_by_uniq_cov, failed_by_min_read, n_valid;
    uint32_t bin_width, min_reads, avg_read_len;
    uint32_t profile_count, profile_failed;
    float coverage_cut_off, uniq_coverage_cut_off, expected_coverage;
    uint64_t n_records, n_targets; /* records pushed; distinct (read, ref) pairs */
    uint64_t total_bins;           /* sum over refs of len/bin_width + 1 */
} slimm_stats;
int slimm_get_stats(slimm_ctx* ctx, slimm_stats* out);

/* Per-reference columns; any pointer may be NULL.  All arrays [n_refs]. */
typedef struct {
    uint32_t* reads_count;
    uint32_t* uniq_reads_count;
    uint32_t* uniq_reads_count2;
    uint32_t* nbins;
    uint32_t* nz_cov;       /* cov.none_zero_bin_count() */
    uint32_t* nz_uniq_cov;
    uint32_t* nz_uniq_cov2;
    uint8_t* valid;         /* member of valid_ref_ids */
    float* abundance;       /* src/slimm.hpp:266-279 */
    float* uniq_abundance;  /* src/slimm.hpp:287-300 */
} slimm_ref_columns;
int slimm_get_ref_columns(slimm_ctx* ctx, slimm_ref_columns* out);

/* Coverage bins of every reference, concatenated without padding in refID order (total_bins words).
 * which: 0 = cov, 1 = uniq_cov, 2 = uniq_cov2 (reference_contig.hpp:110-112). */
int slimm_get_bins(slimm_ctx* ctx, int which, uint32_t* out);

/* The reads' target lists after phase A (the reference's `reads[*].targets`, src/read_stat.hpp:46-59, 61-74): one entry
 * per distinct (read, reference) pair, the targets of a read contiguous, reads in the order the device emitted them.
 *   ref[i]   reference id | bit 31: first target of its read
 *   gbin[i]  bin of the pair's first record, counted over all references (bins of the references before it included,
 *            every reference padded to a multiple of 4 bins) | bit 31: the read has this one target only
 * Call with ref = gbin = NULL to get the number of entries in *n; otherwise cap entries are available and *n are written. */
int slimm_get_read_targets(slimm_ctx* ctx, uint32_t* ref, uint32_t* gbin, uint64_t cap, uint64_t* n);
/* Diagnostic: the width in bits of a target's reference word in device memory -- 16 for a database of at most 32768
 * references (15 bits of reference and the flag), 32 otherwise.  slimm_get_read_targets gives the 32-bit form either way. */
int slimm_target_ref_bits(slimm_ctx* ctx);

/* taxon_id__read_count (src/slimm.hpp:126). stage 0: direct LCA hits only (:536-557); 1: final (:560-610). */
int slimm_taxon_count_size(slimm_ctx* ctx, int stage, uint32_t* n);
int slimm_get_taxon_counts(slimm_ctx* ctx, int stage, uint32_t* taxid, uint32_t* count);
/* taxon_id__children (src/slimm.hpp:127) flattened to (taxid, ref) pairs, sorted. */
int slimm_children_pairs_size(slimm_ctx* ctx, int stage, uint64_t* n);
int slimm_get_children_pairs(slimm_ctx* ctx, int stage, uint32_t* taxid, uint32_t* ref);

/* ---- measurement ---- */
/* When enabled, every kernel launch is bracketed by HIP events on the context's stream. */
int slimm_enable_kernel_timing(slimm_ctx* ctx, int on);
/* Restrict the bracketing to one kernel (a name slimm_kernel_times reports); NULL or "" = all kernels again.  Events
 * cost a few microseconds of stream idle time each, so a throughput run times only the kernel it reports on. */
int slimm_time_only_kernel(slimm_ctx* ctx, const char* name);
/* Names (static strings) and accumulated milliseconds / launch counts since the last call with reset != 0. */
int slimm_kernel_times(slimm_ctx* ctx, const char** names, double* ms, uint32_t* launches, uint32_t cap,
                       uint32_t* n, int reset);

/* Which count the tile bucketing of the last file took in phase A (out[0..2]) and phase B (out[3..5]):
 *   stride     1: every value counted, the buckets laid out back to back; S > 1: every S-th slot counted, the buckets laid
 *              out with capacities ("the sampled count"); 0: the layout has no buckets (direct atomics).  Before the
 *              context's first file: 1
 *   fallback   1: a capacity did not hold and the exact chain behind the attempt placed the buckets (S > 1 only)
 *   peak       the fullest stretch of the attempt, fill / capacity in 1/1024 (above 1024: the one that did not fit)
 * Waits for the context's stream.  SLIMM_FORCE sample_stride=S, sample_k=K choose S and the head-room for a test. */
int slimm_get_bucket_sampling(slimm_ctx* ctx, uint32_t out[6]);

/* Diagnostic for record_order = SLIMM_ORDER_ANY: the stream as the device grouped it by read identity for the front end
 * (after slimm_analyze_alignments): per mapped record its identity (qName key << 2 | mate number, src/slimm.hpp:204-208),
 * reference and global bin, records of one identity adjacent and in file order.  Copies min(cap, *n) records to host
 * arrays (any of which may be NULL); *n = the number of mapped records. */
int slimm_grouped_records(slimm_ctx* ctx, uint64_t* ident, uint32_t* ref, uint32_t* gbin, uint64_t cap, uint64_t* n);
/* The grouping's plan for a stream of n_records (record_order = SLIMM_ORDER_ANY): counting passes over the records, bits
 * per pass, hash bits that make a bucket (= passes * width), persistent workgroups per pass. */
void slimm_group_plan(uint64_t n_records, uint32_t* passes, uint32_t* width, uint32_t* bits, uint32_t* grid);

/* ---- host-only helpers (no GPU needed; used by the host driver and testable on CPU) ---- */
/* get_avg_read_length (src/misc.hpp:509-522). Returns 0 when no record has a sequence (the reference divides by 0). */
uint32_t slimm_host_avg_read_length(const uint32_t* l_seq, uint64_t n, uint32_t sample_size);
/* get_quantile_cut_off<float> (src/misc.hpp:197-216), float32, same operation order. */
float slimm_host_quantile_cut_off(const float* v, uint32_t n, float q);
/* Bin of one record (src/slimm.hpp:200-201). */
uint32_t slimm_host_bin_of(int32_t begin_pos, uint32_t avg_read_len, uint32_t ref_len, uint32_t bin_width);
/* Canonical identity of one record's read (src/slimm.hpp:204-208, quirk Q18).  The reference keys its reads by the STRING
 * qName + ".1" (flag 0x40) / ".2" (else flag 0x80) / nothing, so a first-in-pair record of read "N" and an unflagged
 * record of a read literally named "N.1" are ONE read.  (base, mate) below is a bijection with those strings:
 *   (name, 1) if flag & 0x40;  (name, 2) else if flag & 0x80;  else (name minus its last two bytes, 1 / 2) if the name
 *   ends in ".1" / ".2";  else (name, 0).
 * Returns the length of the base and, in *flag_out, the flag with the mate bit the base carries.  A producer hashes (or
 * compares) name[0, base) and hands the library *flag_out: then "equal keys and equal mate <=> equal reference key
 * string" holds.  The library's own readers (host/alignment_file.cpp, bam_decode.hip) do exactly this. */
uint32_t slimm_host_canonical_read_name(const char* name, uint32_t name_len, uint16_t flag, uint16_t* flag_out);
/* Q18 for a producer of GROUPED records (see "Q18 ON A GROUPED STREAM" above): one slimm_q18_runs per file, zeroed;
 * slimm_host_q18_note for EVERY record in file order -- starts_run: its canonical base differs from the base of the record
 * before it (the file's first record: 1), shortened: slimm_host_canonical_read_name returned less than name_len --;
 * slimm_host_q18_regroup_needed != 0 at the end of the file: some run holds shortened names only, declare the file
 * SLIMM_ORDER_ANY.  (What the device decoders count: slimm_amd/csrc/kernels.h, BamCarry.) */
typedef struct slimm_q18_runs {
    uint64_t short_starts;    /* runs whose first record has a shortened name */
    uint64_t short_to_plain;  /* steps from a shortened to an un-shortened name inside a run */
    int last_short;           /* the record before was shortened */
} slimm_q18_runs;
void slimm_host_q18_note(slimm_q18_runs* q, int starts_run, int shortened);
int slimm_host_q18_regroup_needed(const slimm_q18_runs* q);
/* The same two counts of the file a context's device decoders have read so far (0, 0 for any other record form). */
int slimm_get_q18_runs(slimm_ctx* ctx, uint64_t* short_starts, uint64_t* short_to_plain);
/* ---- THE RECORD FILTER (slimm_amd/csrc/record_filter.h holds the one definition): which alignment records the readers of
 * a file's BYTES leave out -- what samtools view takes as -q, -f and -F, plus a least number of aligned bases and a least
 * identity.  A filtered record is handed on as NOT MAPPED (flag | 0x4; run-marked form: reference word 0), so it is what a
 * copy of the file without that record's alignment would give.  An all-zero filter is off.
 *   A record is JUDGED only if its own 0x4 bit is clear; the flag judged is the file's (not the mate bit Q18 derives from a
 *   name).  The criteria are tried in this order -- flags, MAPQ, aligned length, identity -- and a dropped record is counted
 *   under the first it fails.
 *   aligned = M + = + X bases, columns = M + = + X + I + D of the CIGAR FIELD (a long CIGAR kept in a CG tag is not
 *   followed); "*" / no op: 0 and 0, which fails any min_aligned > 0 and any min_identity_permille > 0.
 *   identity: the record passes iff NM is present (BAM: of any integer type), columns > 0, NM <= columns and
 *   (columns - NM) * 1000 >= min_identity_permille * columns.  A record without NM (BAM: or with a tag area that does not
 *   parse) fails a non-zero identity threshold and is counted as no_nm as well.
 * The filter is part of a context's configuration: set before a file's first push (afterwards: an error), kept across
 * slimm_reset.  It applies to the byte pushes (slimm_push_bam_bytes, _bgzf_blocks, _sam_bytes, ... every form).  Record
 * ARRAYS carry no MAPQ or CIGAR: there the filter is the producer's job, which calls slimm_host_record_passes_* per record
 * and hands a dropped record on with flag | 0x4.  Filtered records still count toward slimm_record_cap(). */
typedef struct slimm_record_filter {
    uint32_t min_mapq;              /* drop MAPQ < min_mapq (255 is a number like any other, as samtools -q) */
    uint32_t require_flags;         /* drop unless (flag & require) == require   (samtools -f) */
    uint32_t exclude_flags;         /* drop if (flag & exclude) != 0             (samtools -F) */
    uint32_t min_aligned;           /* drop if M + = + X bases < min_aligned */
    uint32_t min_identity_permille; /* 0..1000 */
    uint32_t reserved[3];           /* must be 0 */
} slimm_record_filter;
/* f == NULL: off.  Refused: permille > 1000, flag masks above 0xffff, non-zero reserved words, a file already begun. */
int slimm_set_record_filter(slimm_ctx* ctx, const slimm_record_filter* f);
/* out[] = judged, dropped_flags, dropped_mapq, dropped_aligned, dropped_identity, no_nm, 0, 0 of the file's byte pushes so
 * far (no_nm is a subset of dropped_identity); cleared by slimm_reset.  Member 0 of a group: the sum over the members. */
int slimm_get_record_filter_stats(slimm_ctx* ctx, uint64_t out[8]);
/* One record against a filter, on the host: 1 = keep it as it is, 0 = dropped.  *why (may be NULL): 0 passes, 1 flags,
 * 2 MAPQ, 3 aligned length, 4 identity, 5 identity for want of NM, 6 not judged (its 0x4 bit is set: kept as it is).
 * BAM: `record` is the record behind its block_size word and n_bytes that block_size; SAM: `line` is one alignment line,
 * n_bytes its length without (or with) the newline.  No byte outside [0, n_bytes) is read, whatever the bytes say.
 * -1: a NULL argument or a filter slimm_set_record_filter would refuse. */
int slimm_host_record_passes_bam(const slimm_record_filter* f, const uint8_t* record, uint32_t n_bytes, int* why);
int slimm_host_record_passes_sam(const slimm_record_filter* f, const char* line, uint32_t n_bytes, int* why);
/* hipDeviceReset() of the process's devices: for a host about to leave the process.  Contexts must not be used afterwards. */
int slimm_shutdown(void);
/* Library build info. */
/* ---- Several GPUs in one process (slimm_amd/csrc/group.hip): a group of contexts, one per device, used like one.
 * Records are dealt to the members by read as they are pushed (name-grouped streams: contiguous stretches of the file cut
 * at qName-run boundaries, member after member; any other order: key mod n); slimm_group_get_profiles runs the phases on
 * every member with the two exchanges of the multi-rank path in between -- ncclAllGather of the coverage summaries,
 * ncclAllReduce of the partial results, both enqueued on the members' own streams (RCCL is dlopen()ed when the group is
 * created; without it, or when one device is named several times, the same collectives are device-to-device copies and
 * a summing kernel) -- and writes the profile from member 0.  cfg->device is ignored; results (slimm_get_stats,
 * slimm_get_ref_columns, ...) are read from slimm_group_context(g, 0), whose per-reference columns, scalars and
 * per-taxon counts are the merged ones.  The coverage arrays stay per-member partial sums.  Member 0 is also the one
 * that propagates: slimm_set_propagation_walk / _priority are set on it and slimm_get_propagation_order is read from it. */
typedef struct slimm_group slimm_group;
int slimm_group_create(const slimm_config* cfg, const int* devices, uint32_t n_devices, slimm_group** out);
void slimm_group_destroy(slimm_group* g);
const char* slimm_group_last_error(const slimm_group* g); /* g may be NULL: error of the last failed slimm_group_create */
uint32_t slimm_group_size(const slimm_group* g);
slimm_ctx* slimm_group_context(slimm_group* g, uint32_t i);
int slimm_group_uses_rccl(const slimm_group* g);
int slimm_group_reset(slimm_group* g);
/* slimm_set_record_filter on every member (a file split over the members is filtered by each in its own range; the stats
 * are read from member 0, which sums them). */
int slimm_group_set_record_filter(slimm_group* g, const slimm_record_filter* f);
int slimm_group_push_records(slimm_group* g, const uint64_t* read_key, const int32_t* ref_id, const int32_t* begin_pos,
                             const uint16_t* flag, uint64_t n);
/* Packed 16-byte records (slimm_push_records_packed; the identity of a read name is the key's low 61 bits). */
int slimm_group_push_records_packed(slimm_group* g, const uint64_t* packed_key, const int32_t* ref_id, const int32_t* begin_pos,
                                    uint64_t n);
/* Run-marked 8-byte records (slimm_push_records_marked; groups created for grouped input): whole runs go to one member. */
int slimm_group_push_records_marked(slimm_group* g, const uint32_t* word, const int32_t* begin_pos, uint64_t n);
/* With a check word per record (slimm_push_records_checked): two names that collide in the key land on the same member
 * whichever way the records are dealt, so a group reports SLIMM_E_KEY_COLLISION exactly where one context would. */
int slimm_group_push_records_checked(slimm_group* g, const uint64_t* read_key, const int32_t* ref_id, const int32_t* begin_pos,
                                     const uint16_t* flag, const uint32_t* check, uint64_t n);
/* The exchange between phase A and the cut-offs: SUMMARY = ncclAllGather of [per-reference sums | scalars | one bit per
 * bin]; SLICED = all-to-all of the bitmaps in one slice per member (ncclSend / ncclRecv in one group) + a small
 * ncclAllReduce; BINS = the ncclAllReduce(ncclSum) over the integer coverage bins themselves [cov | uniq_cov | scalars],
 * after which -- and after a second all-reduce of uniq_cov2 behind phase B -- every member's slimm_get_bins returns the
 * GLOBAL arrays (what the reference's -ro / -co outputs read, src/slimm.hpp:846-943; nz_uniq_cov2 of
 * slimm_get_ref_columns stays the member's own count: count the non-zero bins of the global array instead).
 * AUTO (default) = SUMMARY up to two members, SLICED above. */
enum { SLIMM_EXCHANGE_AUTO = 0, SLIMM_EXCHANGE_SUMMARY = 1, SLIMM_EXCHANGE_SLICED = 2, SLIMM_EXCHANGE_BINS = 3 };
int slimm_group_set_exchange(slimm_group* g, int mode);
int slimm_group_exchange(const slimm_group* g); /* the form in effect (what AUTO resolves to) */
int slimm_group_get_profiles(slimm_group* g, const char* path); /* path may be NULL; SLIMM_E_NO_HITS like slimm_get_profiles */
/* ONE FILE SPLIT BY BYTE RANGE over a group (files GROUPED by read name or in ANY order): every member reads, inflates and decodes its own contiguous
 * range of the file at once.  Five forms of file: BAM, SAM text, SAM text in BGZF blocks (bgzip), bzip2-compressed SAM
 * text (below: "bzip2 SAM by byte range") and zstd-compressed SAM text of several frames (below: "zstd SAM by byte range").
 * gzip-compressed SAM text is cut at the bits where blocks start and read in two passes (below: "gzip SAM by byte range").
 * (A zstd file of one frame cannot be cut: it goes through one member.)
 *   The plan (host only, no GPU): offsets_out[0, n]; range i = [offsets_out[i], offsets_out[i + 1]), ranges may be empty.
 * slimm_host_bgzf_ranges -- BAM and BGZF SAM --: offsets_out[0] = 0, offsets_out[n] = the file's size; a range starts on a
 * BGZF block boundary (a header whose next three headers chain through BSIZE + 1, or whose chain reaches the EOF block or
 * the file's end); no cut lies in front of the block that holds inflated byte `skip` (the header's inflated length: member
 * 0 takes all of it and pushes its first blocks with that skip).  slimm_host_text_ranges -- plain SAM --: offsets_out[0] =
 * skip, the file offset of the first alignment line, offsets_out[n] = the file's size, the bytes between divided evenly
 * and cut anywhere; SLIMM_E_INVALID for a path that is no regular file or a skip beyond its size.
 *   What a member does FIRST, before its first push: SAM text in either form names its references, so every member gets
 * the header's names with slimm_set_reference_names; every member but the first calls slimm_set_input_mid_file(ctx, 1, ...)
 * and every member but the last (..., 1); slimm_set_input_size_hint(ctx, the range's bytes) sizes a BGZF range's windows.
 * A range that starts inside the file finds its first record in its first window, on the device, and keeps the bytes in
 * front of it -- the head, at most 16 MiB -- there for the member on its left.  BAM: the first record is guessed from the
 * bytes.  SAM: the first line starts behind the first newline, the head is the bytes through that newline (a whole line
 * when the cut fell on a line start), and no newline within 16 MiB of a range's first window that is not also its last is
 * SLIMM_E_SPLIT.  A range that ends inside the file may end inside a record or a line: what is left stays as the carry;
 * an incomplete last line gets no newline there (only the file's last member ends a last line that lacks one; when that
 * member's range holds no text at all -- it is empty, or a BGZF EOF block only -- the stitch ends the line instead).
 *   Each member then pushes its range -- slimm_push_bgzf_blocks, slimm_push_sam_bytes or slimm_push_bgzf_sam_blocks, last =
 * 1 at the range's end; an empty range is one push of no bytes with last = 1 -- all members at once, and
 * slimm_group_stitch_ranges joins the cuts on the devices: the bytes around a cut are decoded by the member on its left,
 * which must end exactly where the right member's first record begins (otherwise SLIMM_E_SPLIT: read the file through
 * member 0 instead); the run of a read name that a cut splits moves, device to device, to the member that holds its
 * start; the Q18 counts are summed over the members (SLIMM_E_REGROUP as for one context).  slimm_group_get_profiles then
 * runs on the members' records as they are (no dealing from member 0).  This is also how ONE device takes a file of more
 * records than one context holds: a group that names the same device several times.
 *   A file in ANY order is planned, announced and pushed in the same way, and slimm_group_stitch_ranges joins the cuts in the
 * same way (SLIMM_E_SPLIT as above).  It has no runs to join and no Q18 counts; instead every member partitions the records
 * of its range by owner -- (key & the 62 identity bits) mod n, the rule of slimm_group_push_records* -- with a stable
 * partition on the device (slimm_partition_by_key), and member j receives stretch j of every member in member order, device
 * to device: all records of a read on one member, in the file's order.  A member with no records, or with a range that is
 * all head, sends and receives empty stretches.  Nothing may have been dealt through slimm_group_push_records* before.
 *   Memory: while the records are dealt every member holds one more copy of its records (22 bytes each, the send buffers);
 * they are released before slimm_group_stitch_ranges (or, through member 0, before phase A) goes on.  A member that receives
 * more records than it decoded grows its record arrays to what it receives.
 *   bzip2 SAM by byte range.  A bzip2 file's blocks start at bit offsets, and nothing in the file says where: the device
 * finds them (their 48-bit magic at every bit offset) and trusts none.  THE RULE OF THE CUT: a block -- or an end-of-stream
 * marker, with the next stream's header behind it -- belongs to the member in whose byte range the first bit of its magic
 * lies.  slimm_host_bzip2_ranges cuts at plain byte offsets: offsets_out[0] = 0, offsets_out[n] = the file's size, the
 * others divide evenly the bytes behind the block that holds decoded byte skip - 1 (the header's last byte: it decodes the
 * file's first blocks on the host to find it; member 0 holds the whole header and pushes with that skip); SLIMM_E_INVALID
 * for something that is no regular file, or does not start a bzip2 stream.  Every member announces its flags with
 * slimm_set_input_mid_file AND its range's absolute file offsets with slimm_set_input_range(ctx, begin, end), and pushes
 * -- slimm_push_bzip2_sam_bytes -- its range PLUS A SLACK behind it, slimm_bzip2_split_slack() bytes or up to the file's
 * end, so that the block that starts inside the range can finish: no compressed byte is handed from member to member.
 *   A range that starts inside the file starts its chain at the first candidate at or behind its first bit that decodes;
 * candidates in front of it that do not are dropped as false magics, and an end-of-stream marker in front of it starts
 * the chain instead.  It does not know its stream's level -- its blocks are decoded with the largest, and the largest one
 * is remembered -- nor the combined CRC so far -- it keeps (number of blocks, partial value from 0) until its first
 * marker.  A mismatch of that first block's CRC is SLIMM_E_SPLIT, not a verdict on the file.  A range that ends inside the
 * file stops at the first block or marker that starts at or behind its end, at last = 1 too, and drops the rest of the
 * slack; a block the slack does not finish is SLIMM_E_SPLIT; a range in which nothing starts decodes nothing and is an
 * empty member.  Error messages name the file's bytes, as for one context.
 *   slimm_group_stitch_ranges first goes left to right over the cuts on host scalars: the left chain must end exactly at
 * the bit where the next member that holds a block starts (SLIMM_E_SPLIT otherwise); that member's blocks of its first
 * stream must fit the level of the left chain's stream ("block longer than its stream's level allows"); and the combined
 * CRC is linear -- c = rotl(c, 1) ^ crc per block --, so rotl^k(left's value) ^ the member's partial value must be the
 * CRC of its first marker ("combined CRC mismatch", with the marker's byte), or is handed on to the next cut when it saw
 * none.  The decoded text is then stitched as SAM text is: a member's text starts at a block boundary inside a line, and
 * its head through the first newline goes to the member on its left.
 *   zstd SAM by byte range.  A zstd file is cut where a frame -- or a skippable frame -- starts, and nowhere else: frames
 * are byte-aligned, start with a magic and are independent of each other (window, repeat offsets and entropy tables start
 * afresh at a frame header), which is what pzstd, the seekable format and `cat a.zst b.zst` write.  A single frame cannot be
 * cut: its copies reach back through the whole window.  slimm_host_zstd_ranges: offsets_out[0] = 0, offsets_out[n] = the
 * file's size, every other offset the first byte of a frame or of a skippable frame, or the file's size.  No cut lies in
 * front of the end of the frame that holds decoded byte skip - 1 (the header's frames are decoded on the host; member 0
 * holds the whole header and pushes with that skip).  Cut i is the earliest start at or behind first + i * (size - first) /
 * n that passes these checks: the frame header parses (reserved bit, window of at most 128 MiB, dictionary id 0), the block
 * chain reaches a last block with no block of the reserved type and none above the frame's block maximum, a stated
 * checksum fits in the file, and behind it the file ends or a frame's or skippable frame's magic stands (a skippable
 * frame: its length fits, and the same holds behind it).  The search gives up 64 MiB behind its target (a design constant
 * that bounds the planner's reading; SLIMM_FORCE zstd_cut_search=N): the cut is then the next one found, or the file's
 * size, and the range in between is empty -- so a file of one frame has every cut at its size.  SLIMM_E_INVALID for a skip
 * of 2^32 or more, for a path that is no regular file, and when the header's frames do not decode.  The planner trusts
 * nothing it cannot walk; the members and the stitch check the rest.
 *   Every member announces its flags with slimm_set_input_mid_file AND its range with slimm_set_input_range(ctx, begin,
 * end), and pushes -- slimm_push_zstd_sam_bytes, skip for member 0 only -- exactly its range: there is no slack.  A range
 * that starts inside the file whose first bytes start no frame is SLIMM_E_SPLIT; so is a range that ends inside the file
 * and at last = 1 does not stand between frames with every byte read ("the range does not end at a frame boundary": a
 * frame or block that runs past the range).  The file's last member keeps the truncation errors of one context.  Nothing
 * in front of the range exists for the member; content sizes and checksums are checked by the member that owns the
 * frame, and error messages name the file's bytes.  An empty range, or one of skippable and empty frames only, decodes no
 * text and is an empty member.  slimm_get_zstd_stats stays per context: the members' counters sum to the file's.
 *   slimm_group_stitch_ranges first checks on host scalars, left to right, that every member's decoder stopped between
 * frames exactly at its range's end (SLIMM_E_SPLIT names the member); the text is then stitched as SAM text is.
 * slimm_zstd_split_floor(): the least bytes per member -- (size - first cut) / members -- at which the command cuts a
 * zstd file for --split-input: the codec's round size, 32 MiB (a member with less decodes its range in one round, and no
 * gain from that has been measured: a stated default, not a measurement; SLIMM_FORCE zstd_split_floor=N). */
int slimm_host_zstd_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out);
uint64_t slimm_zstd_split_floor(void);
/*   xz SAM by byte range.  An xz file is cut where its indexes say so, and nothing is guessed: the index at each stream's
 * end states every block's unpadded size and text size, blocks are byte-aligned, and a block needs nothing of the one in
 * front (dictionary and state are reset at its first chunk).  slimm_host_xz_ranges reads only the file's tail or tails --
 * footer, index and stream header, stream by stream from the file's end -- and decodes nothing: offsets_out[0] = 0,
 * offsets_out[n] = the file's size, every other offset the first byte of a block that is not the first of its stream, the
 * first byte of a stream header (the cut in front of a stream's first block; stream padding belongs to the member on the
 * left), or the file's size.  No cut lies in front of the end of the block that holds decoded byte skip - 1, found from
 * the indexes' cumulative text sizes (member 0 holds the whole header and pushes with that skip).  Cut i is the earliest
 * legal cut at or behind first + i * (size - first) / n; the indexes are complete, so no search gives up, and more members
 * than blocks get empty ranges.  SLIMM_E_INVALID for a path that is no regular file, an index that does not parse, a skip
 * of 2^32 or more, and a skip beyond the text the indexes state.
 *   A range that starts at a block inside a stream has not seen that stream's header, so it does not know the check kind,
 * which also sizes the field behind every block.  slimm_host_xz_check_at(path, offset, &check): -1 when offset is 0, a
 * stream header's first byte or no byte of a stream, else the check id of the stream around it, from its footer.  Every
 * member announces its flags with slimm_set_input_mid_file, its range with slimm_set_input_range(ctx, begin, end) AND that
 * check with slimm_set_xz_range_check(ctx, check) (-1, the default: none told), all before its first window, and pushes --
 * slimm_push_xz_sam_bytes, skip for member 0 only -- exactly its range: there is no slack.  With a told check the walk
 * starts among the stream's blocks, without one at a stream header; a first byte that starts neither is SLIMM_E_SPLIT.  So
 * is a range that ends inside the file and at last = 1 does not stand exactly at its end, at a block's first byte or
 * between streams ("the range does not end at a block boundary").  The file's last member keeps the truncation errors of
 * one context.  Nothing in front of the range exists for the member, and error messages name the file's bytes.  The member
 * in whose range a stream's index lies reads it and the footer: it checks the index's last k records against its own k
 * blocks of that stream and keeps the first N - k for the stitch; a footer of another check kind than the told one is
 * SLIMM_E_SPLIT.  An empty range is an empty member.  slimm_get_xz_stats stays per context and the members' counters sum to
 * the file's: a stream is counted by the member that read its header, index records by the member that read the index.
 *   slimm_group_stitch_ranges first checks on host scalars, left to right: every member's walker stopped exactly at its
 * range's end (SLIMM_E_SPLIT names the member); a member that was told a check has a stream open across the cut in front
 * of it, of that kind (SLIMM_E_SPLIT); the (unpadded size, text size) pairs of the left members' blocks of that stream
 * equal, in order and in number, the records the member that met the index kept (SLIMM_E_INVALID "index does not match the
 * blocks") -- so every index record of the file is checked against its block exactly once.  The text is then stitched as
 * SAM text is.  slimm_xz_split_floor(): the least blocks per member -- the blocks behind the first legal cut / members --
 * at which the command cuts an xz file for --split-input: 16, the command's default for reading an xz file on the device at
 * all, since a range is decoded a lane per block as a file is (a stated default, NOT a measurement; SLIMM_FORCE
 * xz_split_blocks=N). */
int slimm_host_xz_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out);
int slimm_host_xz_check_at(const char* path, uint64_t offset, int* check_out);
int slimm_set_xz_range_check(slimm_ctx* ctx, int check);
uint64_t slimm_xz_split_floor(void);
/*   gzip SAM by byte range.  A deflate stream has no marks, its blocks start at any bit, and a block copies from the 32 768
 * bytes of text in front of it, whatever block they came from -- in SAM text those bytes never die out: a constant tag is
 * copied from its previous copy for the whole file.  So a gzip file is cut at BITS and read in two passes.
 *   The plan.  slimm_host_gzip_ranges: bit_offsets_out[0] = 0, bit_offsets_out[n] = 8 x the file's size; member i reads the
 * file's bytes [bits[i] / 8, (bits[i + 1] + 7) / 8), so neighbours share at most one byte.  No cut lies in front of the end
 * of the block that holds inflated byte skip - 1 (the file's first blocks are inflated on the host; member 0 holds the
 * whole header and pushes with that skip).  Cut i is the first bit at or behind its even share of the bits behind that floor
 * at which a non-final dynamic block that zlib would take starts (the two codes parse, the literal/length code complete)
 * AND a walk from there -- Huffman codes only -- passes 4 further block boundaries, or a final block, without an error.  The
 * walk also ends after 4 MiB of compressed bytes; the candidate then counts if at least one boundary was passed.  The
 * search gives up 64 MiB behind its target: the cut is then the next one found, or the file's end, and the range in
 * between is empty -- a stream of stored or fixed blocks only has every cut at the file's end.  (4 blocks, 64 MiB: stated
 * defaults, not measurements; SLIMM_FORCE gzip_cut_blocks=N, gzip_cut_search=N.)  SLIMM_E_INVALID for a path that is no
 * regular file, bytes that start no gzip member, a header that does not inflate, a skip of 2^32 or more.  The planner trusts
 * nothing it cannot walk: a cut it took can still be false, and the members and the stitch decide.
 *   Every member announces its flags with slimm_set_input_mid_file AND its range with slimm_set_gzip_range(ctx, begin_bit,
 * end_bit) before its first push, and pushes -- slimm_push_gzip_sam_bytes, skip for member 0 only -- the bytes that hold
 * its bits.  A range that starts inside the file starts among a gzip member's blocks at begin_bit: no member header is
 * expected, 32 768 bytes of that member are taken to lie in front until slimm_group_gzip_windows knows better, and its CRC
 * register and member length start at 0 (a partial).  A range that ends inside the file starts no chunk at or behind
 * end_bit, its size pass stops there, and it is done when its chain stands exactly on end_bit; a chain that steps over
 * end_bit, or has not reached it at last = 1, is SLIMM_E_SPLIT and names the bit.  An error among the blocks of the gzip
 * member a range started in is SLIMM_E_SPLIT too, no verdict on the file: the range may have started where no block does.
 *   THE WINDOW PASS: slimm_set_gzip_window_pass(ctx, 1) before the first push, then the same pushes of the same bytes.  The
 * rounds find, walk, chain and decode as ever; instead of resolving the text they propagate the last 32 768 symbols chunk by
 * chunk in 16 bits, each a byte or a marker for a byte of the 32 768 in front of the RANGE.  No text, no records, no CRC;
 * memory is that of one round, whatever the range's size.  slimm_group_gzip_windows(g) then goes left to right: member k's
 * chain ended on member k + 1's begin_bit (SLIMM_E_SPLIT); its final window, its markers filled from the bytes in front of
 * its own range by a tiny kernel, is copied device to device and becomes the bytes in front of member k + 1, with how many
 * of them belong to the open gzip member; every member's file state is made fresh, its announcements kept.  The last
 * member need not run the window pass.  The serial work is 32 KiB per cut.
 *   THE TEXT PASS is the pipeline of one context from the installed bytes: the same pushes once more.  It must reproduce
 * the window pass's end bit and text length (SLIMM_E_SPLIT).  A member that starts inside a gzip member cannot check that
 * member's trailer: at the first trailer in its range it keeps its partial register and length and the trailer's CRC32,
 * ISIZE and byte offset; later gzip members it checks itself.  Text, heads and carries are SAM text's.
 *   slimm_group_stitch_ranges first goes left to right on host scalars: every chain ended on its range's end; the register
 * of a gzip member that lies over cuts is folded, s = s * x^(8 len_k) + partial_k, and held with the summed length against
 * the trailer that member k read -- "corrupt gzip stream (incorrect data check)" or "(incorrect length check)" with the
 * trailer's byte, SLIMM_E_INVALID; a range without a trailer hands both on.  slimm_get_gzip_stats stays per context and the
 * members' counters sum to the file's: a gzip member is counted by whoever read its trailer, a block by exactly one member.
 * slimm_gzip_split_floor(): the least bytes per member -- (size - first cut) / members -- at which the command cuts a gzip
 * file for --split-input: 32 MiB as zstd's (a stated default, not a measurement; SLIMM_FORCE gzip_split_floor=N). */
int slimm_host_gzip_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* bit_offsets_out);
int slimm_set_gzip_range(slimm_ctx* ctx, uint64_t begin_bit, uint64_t end_bit);
int slimm_set_gzip_window_pass(slimm_ctx* ctx, int on);
int slimm_group_gzip_windows(slimm_group* g);
uint64_t slimm_gzip_split_floor(void);
int slimm_host_bzip2_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out);
/* A range's absolute file offsets [begin, end) (bzip2 SAM, zstd SAM, xz SAM; before the range's first window, beside slimm_set_input_mid_file) */
int slimm_set_input_range(slimm_ctx* ctx, uint64_t begin, uint64_t end);
/* the bytes a member reads behind its range of a bzip2 file (slimm_amd/csrc/bzip2_block.h: kSplitSlack, from the format's bounds) */
uint64_t slimm_bzip2_split_slack(void);
int slimm_host_bgzf_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out);
int slimm_host_text_ranges(const char* path, uint64_t skip, uint32_t n, uint64_t* offsets_out);
int slimm_set_input_mid_file(slimm_ctx* ctx, int starts_mid_file, int ends_mid_file);
int slimm_group_stitch_ranges(slimm_group* g);
/* the most records one context takes (below 2^31; SLIMM_FORCE record_cap=N lowers it, for tests) */
uint64_t slimm_record_cap(void);
/* A GROUPED file may also reach a group through ONE member: push its windows to slimm_group_context(g, 0) (slimm_push_bam_bytes /
 * _bgzf_blocks / _sam_bytes: the device inflates and decodes at the single-context rate) and nothing through
 * slimm_group_push_records*; slimm_group_get_profiles then deals member 0's run-marked records to the members in contiguous
 * stretches cut at qName-run starts, device to device (8 bytes per record), before phase A.  SLIMM_E_REGROUP from member 0
 * (Q18) comes back as the group's return code: such a file goes through slimm_group_push_records* in any order.
 *   A file in ANY order reaches a group through member 0 in the same way (slimm_push_bam_bytes / _bgzf_blocks / _sam_bytes /
 * _bgzf_sam_blocks / _bzip2_sam_bytes to slimm_group_context(g, 0), nothing through slimm_group_push_records*): when only member
 * 0 holds records, in the four-array form, slimm_group_get_profiles partitions them by owner on the device (key mod n, the
 * rule of slimm_group_push_records*), copies stretch i to member i device to device with its check words -- member 0 keeps
 * stretch 0 -- and releases the send buffers (one more copy of the records, 22 bytes each) before phase A.  The records
 * and stretch lengths do not depend on whether RCCL was loaded: the deal is copies in either case. */

/* Starts the HIP runtime on `device` (what the first slimm_create of a process would otherwise pay, 0.1 - 0.3 s): for
 * hosts that call it from a thread of their own while they load their database and open their input. */
int slimm_warm_up(int device);
const char* slimm_version(void);

/* BGZF blocks inflated on the device, by themselves: `blocks` = n_bytes of whole BGZF blocks (gzip members with the BC
 * extra field, as in a .bam / .bgz file) in host memory, one behind the other; their inflated bytes, one block's behind the
 * other's, go to out[0, *out_bytes) in host memory (slimm_amd/csrc/bgzf_tokens.hip, bgzf_inflate.hip); ISIZE, the
 * well-formedness of every DEFLATE block and the CRC32 of the gzip trailer are checked.  *kernel_ms (may be null): the
 * inflate kernel alone.  Errors (-1 bad input / a corrupt block, -2 HIP) come with a message in err[0, err_cap).
 * Replaces, together with slimm_push_bam_bytes, what seqan::BamFileIn does for the reference (call sites src/misc.hpp:498-522,
 * src/slimm.hpp:194-208).  slimm_push_bgzf_blocks feeds a context's record stream the same way without the round trip. */
int slimm_bgzf_inflate(int device, const uint8_t* blocks, uint64_t n_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes,
                       double* kernel_ms, char* err, uint64_t err_cap);
/* The same with the choice of kernels and a count.  how = 0: the two-phase kernels (slimm_amd/csrc/bgzf_tokens.hip: a lane per
 * block decodes the Huffman codes into literals in place + match tokens, a workgroup per block fills the matches in LDS and
 * checks the CRC), with the lane-per-block kernel behind them for what they hand over -- blocks with a stored DEFLATE block
 * inside, and anything irregular; how = 1: the lane-per-block kernel for every block.  *lane_blocks (may be null): the blocks
 * the lane-per-block kernel inflated. */
int slimm_bgzf_inflate_with(int device, const uint8_t* blocks, uint64_t n_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes,
                            double* kernel_ms, char* err, uint64_t err_cap, uint32_t how, uint32_t* lane_blocks);
/* The stable partition of four-array records by owner, by itself (slimm_amd/csrc/deal_by_key.hip): the kernels a group of
 * m members runs to give every read of a file in any order to one member.  Host arrays in and out, n < 2^31 records each,
 * 1 <= m <= 255; check / check_out may be NULL.  The outputs hold the same records in m contiguous stretches, stretch o =
 * exactly the records with (key & (2^62 - 1)) % m == o in their input order; counts_out[o] = its length.  *kernel_ms (may be
 * null): the three kernels alone (count, scan, scatter).  Errors (-1 bad input, -2 HIP) come with a message in err[0, err_cap). */
int slimm_partition_by_key(int device, const uint64_t* key, const int32_t* ref, const int32_t* pos, const uint16_t* flag,
                           const uint32_t* check, uint64_t n, uint32_t m, uint64_t* key_out, int32_t* ref_out, int32_t* pos_out,
                           uint16_t* flag_out, uint32_t* check_out, uint64_t* counts_out, double* kernel_ms, char* err, uint64_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* SLIMM_HIP_H */
