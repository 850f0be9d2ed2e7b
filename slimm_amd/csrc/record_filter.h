// The record filter: which alignment records a reader leaves out, said once for the host reader (host/alignment_file.cpp),
// the device decoders (bam_decode.hip, sam_decode.hip) and a producer of record arrays (slimm_host_record_passes_*).
//
// A filtered record is a record the reader hands on as NOT MAPPED (flag bit 0x4 / reference word 0): the reference's loop
// skips such a record (src/slimm.hpp:197) and so does everything behind the decoders.  What samtools view takes as -q, -f,
// -F, plus a least number of aligned bases and a least identity over the alignment's columns.
//
// A record is JUDGED only if its own 0x4 bit is clear.  The criteria are tried in a fixed order -- flags, MAPQ, aligned
// length, identity -- and a dropped record is counted under the first it fails, so the counts add up and host and device
// agree on them.  The flag judged is the flag as it stands in the file (not the mate bit Q18 derives from a name:
// read_identity.h).
//   aligned = M + = + X bases; columns = M + = + X + I + D.  A CIGAR of "*" (BAM: no op) gives 0 and 0.
//   identity: passes iff NM is there, columns > 0, NM <= columns and (columns - NM) * 1000 >= permille * columns --
//   integers only, so that no float can differ between host and device.
// BAM: the CIGAR field is judged (a long CIGAR kept in a CG tag is not followed); NM is found by walking the tag area,
// of any integer type; a tag area that does not parse counts as "NM absent".  Every read stays inside the record.
// SAM: MAPQ is field 5, CIGAR field 6 (decimal runs and op letters; any other byte: judged as "*"), NM the first "NM:i:"
// field from field 12 on.  Every read stays in front of the line's newline and of `end`.
#pragma once
#include <stdint.h>

#include "../../include/slimm_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SLIMM_RF_FN __host__ __device__ inline
#else
#define SLIMM_RF_FN inline
#endif

/* what became of a record (the `why` of slimm_host_record_passes_*); 1..5 are drops, NO_NM counts under identity too */
enum {
    SLIMM_RF_PASS = 0,
    SLIMM_RF_FLAGS = 1,
    SLIMM_RF_MAPQ = 2,
    SLIMM_RF_ALIGNED = 3,
    SLIMM_RF_IDENTITY = 4,
    SLIMM_RF_NO_NM = 5,
    SLIMM_RF_NOT_JUDGED = 6
};
/* the counters of slimm_get_record_filter_stats */
enum { SLIMM_RF_N_JUDGED = 0, SLIMM_RF_N_FLAGS, SLIMM_RF_N_MAPQ, SLIMM_RF_N_ALIGNED, SLIMM_RF_N_IDENTITY, SLIMM_RF_N_NO_NM, SLIMM_RF_N_STATS = 8 };

SLIMM_RF_FN int slimm_rf_on(const slimm_record_filter* f) {
    return (f->min_mapq | f->require_flags | f->exclude_flags | f->min_aligned | f->min_identity_permille) != 0u;
}
SLIMM_RF_FN int slimm_rf_dropped(int why) { return why >= SLIMM_RF_FLAGS && why <= SLIMM_RF_NO_NM; }
/* permille <= 1000, flag masks <= 0xffff, reserved 0 */
SLIMM_RF_FN int slimm_rf_valid(const slimm_record_filter* f) {
    return f->min_identity_permille <= 1000u && f->require_flags <= 0xffffu && f->exclude_flags <= 0xffffu && f->reserved[0] == 0u &&
           f->reserved[1] == 0u && f->reserved[2] == 0u;
}

/* what the 32 fixed bytes (the first five fields) decide: NOT_JUDGED, FLAGS, MAPQ, or PASS so far */
SLIMM_RF_FN int slimm_rf_head(const slimm_record_filter* f, uint32_t flag, uint32_t mapq) {
    if (flag & 0x4u) return SLIMM_RF_NOT_JUDGED;
    if ((flag & f->require_flags) != f->require_flags || (flag & f->exclude_flags) != 0u) return SLIMM_RF_FLAGS;
    if (mapq < f->min_mapq) return SLIMM_RF_MAPQ;
    return SLIMM_RF_PASS;
}
SLIMM_RF_FN int slimm_rf_needs_cigar(const slimm_record_filter* f) { return (f->min_aligned | f->min_identity_permille) != 0u; }
/* ... and the rest: aligned length, then identity */
SLIMM_RF_FN int slimm_rf_tail(const slimm_record_filter* f, uint64_t aligned, uint64_t columns, int has_nm, uint64_t nm) {
    if (aligned < f->min_aligned) return SLIMM_RF_ALIGNED;
    if (f->min_identity_permille) {
        if (!has_nm) return SLIMM_RF_NO_NM;
        if (columns == 0u || nm > columns || (columns - nm) * 1000u < (uint64_t)f->min_identity_permille * columns) return SLIMM_RF_IDENTITY;
    }
    return SLIMM_RF_PASS;
}

/* ---- BAM: r = the record behind its block_size word, n = block_size ---- */
SLIMM_RF_FN uint32_t slimm_rf_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
SLIMM_RF_FN uint32_t slimm_rf_u32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
/* bytes of a tag value of integer / float type t; 0: not such a type */
SLIMM_RF_FN uint32_t slimm_rf_scalar_size(uint32_t t) {
    return (t == 'A' || t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : (t == 'i' || t == 'I' || t == 'f') ? 4u : 0u;
}
/* the tag area r[p, n): NM's value -> *nm, 1; 0: no NM, or the area does not parse */
SLIMM_RF_FN int slimm_rf_bam_nm(const uint8_t* r, uint64_t p, uint64_t n, uint64_t* nm) {
    while (p + 3u <= n) {
        const uint32_t t0 = r[p], t1 = r[p + 1u], ty = r[p + 2u];
        p += 3u;
        const uint32_t sz = slimm_rf_scalar_size(ty);
        if (sz) {
            if (p + sz > n) return 0;
            if (t0 == 'N' && t1 == 'M' && ty != 'A' && ty != 'f') {
                int64_t v;
                if (ty == 'c') v = (int8_t)r[p];
                else if (ty == 'C') v = r[p];
                else if (ty == 's') v = (int16_t)slimm_rf_u16(r + p);
                else if (ty == 'S') v = slimm_rf_u16(r + p);
                else if (ty == 'i') v = (int32_t)slimm_rf_u32(r + p);
                else v = slimm_rf_u32(r + p);
                *nm = (uint64_t)v;   /* (a negative NM: larger than any number of columns) */
                return 1;
            }
            p += sz;
        } else if (ty == 'Z' || ty == 'H') {
            while (p < n && r[p] != 0u) ++p;
            if (p >= n) return 0;   /* (no NUL inside the record) */
            ++p;
        } else if (ty == 'B') {
            if (p + 5u > n) return 0;
            const uint32_t es = slimm_rf_scalar_size(r[p]);
            if (!es || r[p] == 'A') return 0;
            const uint64_t bytes = (uint64_t)slimm_rf_u32(r + p + 1u) * es;
            p += 5u;
            if (bytes > n - p) return 0;
            p += bytes;
        } else {
            return 0;
        }
    }
    return 0;
}
SLIMM_RF_FN int slimm_rf_bam(const slimm_record_filter* f, const uint8_t* r, uint32_t n) {
    if (n < 32u) return SLIMM_RF_NOT_JUDGED;   /* (no record: the reader's error, not the filter's) */
    const int head = slimm_rf_head(f, slimm_rf_u16(r + 14), r[9]);
    if (head != SLIMM_RF_PASS || !slimm_rf_needs_cigar(f)) return head;
    const uint64_t l_name = r[8], n_cigar = slimm_rf_u16(r + 12), l_seq = slimm_rf_u32(r + 16);
    const uint64_t c0 = 32u + l_name, c1 = c0 + 4u * n_cigar;
    uint64_t aligned = 0, columns = 0;
    if (c1 <= n) {
        for (uint64_t p = c0; p < c1; p += 4u) {
            const uint32_t w = slimm_rf_u32(r + p), op = w & 15u;
            const uint64_t len = w >> 4;
            if (op == 0u || op == 7u || op == 8u) aligned += len;             /* M = X */
            if (op == 0u || op == 7u || op == 8u || op == 1u || op == 2u) columns += len;   /* ... I D */
        }
    }
    uint64_t nm = 0;
    int has_nm = 0;
    if (f->min_identity_permille && aligned >= f->min_aligned) {
        const uint64_t tags = c1 + (l_seq + 1u) / 2u + l_seq;
        has_nm = tags <= n ? slimm_rf_bam_nm(r, tags, n, &nm) : 0;
    }
    return slimm_rf_tail(f, aligned, columns, has_nm, nm);
}

/* ---- SAM: s[p, end) from the start of a field on; a field ends at a tab, the line at a newline or `end` ---- */
SLIMM_RF_FN uint64_t slimm_rf_field_end(const uint8_t* s, uint64_t p, uint64_t end) {
    while (p < end && s[p] != '\t' && s[p] != '\n') ++p;
    return p;
}
/* the start of the field behind the one that ends at e; `end`: the line has no further field */
SLIMM_RF_FN uint64_t slimm_rf_next_field(const uint8_t* s, uint64_t e, uint64_t end) { return (e < end && s[e] == '\t') ? e + 1u : end; }
/* flag: the line's FLAG as a number; mapq_at: where field 5 (MAPQ) starts (`end`: the line stops before it) */
SLIMM_RF_FN int slimm_rf_sam(const slimm_record_filter* f, uint32_t flag, const uint8_t* s, uint64_t mapq_at, uint64_t end) {
    const uint64_t cap = 1ull << 40;
    uint64_t p = mapq_at, e = slimm_rf_field_end(s, p, end);
    uint64_t mapq = 0;
    for (uint64_t i = p; i < e && s[i] >= '0' && s[i] <= '9'; ++i) mapq = mapq < cap ? mapq * 10u + (s[i] - '0') : mapq;
    const int head = slimm_rf_head(f, flag, mapq > 0xffffffffull ? 0xffffffffu : (uint32_t)mapq);
    if (head != SLIMM_RF_PASS || !slimm_rf_needs_cigar(f)) return head;
    /* field 6: runs of digits and an op letter each; anything else: "*" */
    p = slimm_rf_next_field(s, e, end);
    e = slimm_rf_field_end(s, p, end);
    uint64_t aligned = 0, columns = 0, run = 0;
    int digits = 0, star = p == e;
    for (uint64_t i = p; i < e && !star; ++i) {
        const uint32_t ch = s[i];
        if (ch >= '0' && ch <= '9') {
            run = run < cap ? run * 10u + (ch - '0') : run;
            digits = 1;
        } else if (digits && (ch == 'M' || ch == '=' || ch == 'X')) {
            aligned += run, columns += run, run = 0, digits = 0;
        } else if (digits && (ch == 'I' || ch == 'D')) {
            columns += run, run = 0, digits = 0;
        } else if (digits && (ch == 'N' || ch == 'S' || ch == 'H' || ch == 'P')) {
            run = 0, digits = 0;
        } else {
            star = 1;
        }
    }
    if (star || digits) aligned = columns = 0;   /* (digits without their op letter at the end: no CIGAR either) */
    uint64_t nm = 0;
    int has_nm = 0;
    if (f->min_identity_permille && aligned >= f->min_aligned) {
        for (int k = 6; k < 11; ++k) {   /* fields 7 .. 11 */
            p = slimm_rf_next_field(s, e, end);
            e = slimm_rf_field_end(s, p, end);
        }
        for (p = slimm_rf_next_field(s, e, end); p < end; p = slimm_rf_next_field(s, e, end)) {
            e = slimm_rf_field_end(s, p, end);
            if (e - p >= 5u && s[p] == 'N' && s[p + 1u] == 'M' && s[p + 2u] == ':' && s[p + 3u] == 'i' && s[p + 4u] == ':') {
                uint64_t i = p + 5u, v = 0;
                const int neg = i < e && s[i] == '-';
                if (i < e && (s[i] == '-' || s[i] == '+')) ++i;
                const uint64_t d0 = i;
                for (; i < e && s[i] >= '0' && s[i] <= '9'; ++i) v = v < cap ? v * 10u + (s[i] - '0') : v;
                has_nm = i > d0;
                nm = (neg && v) ? ~0ull : v;
                break;
            }
        }
    }
    return slimm_rf_tail(f, aligned, columns, has_nm, nm);
}
/* a whole line s[0, n): its FLAG (field 2) read as the readers read it, then slimm_rf_sam */
SLIMM_RF_FN int slimm_rf_sam_line(const slimm_record_filter* f, const uint8_t* s, uint64_t n) {
    uint64_t e = slimm_rf_field_end(s, 0, n);
    uint64_t p = slimm_rf_next_field(s, e, n);
    e = slimm_rf_field_end(s, p, n);
    uint64_t i = p, v = 0;
    while (i < e && s[i] == ' ') ++i;
    int neg = 0;
    if (i < e && (s[i] == '-' || s[i] == '+')) neg = s[i++] == '-';
    for (; i < e && s[i] >= '0' && s[i] <= '9'; ++i) v = v * 10u + (s[i] - '0');
    const uint32_t flag = (uint32_t)(neg ? 0u - v : v) & 0xffffu;
    p = slimm_rf_next_field(s, e, n);                 /* RNAME */
    e = slimm_rf_field_end(s, p, n);
    p = slimm_rf_next_field(s, e, n);                 /* POS */
    e = slimm_rf_field_end(s, p, n);
    return slimm_rf_sam(f, flag, s, slimm_rf_next_field(s, e, n), n);
}

#if defined(__HIPCC__)
/* The device decoders: a lane's verdicts are counted in n[SLIMM_RF_N_NO_NM + 1]; behind the lane's records the wave's sums
 * go to the context's counters -- one atomic per wave and non-zero count.  Called by every lane of a wave of 64. */
__device__ inline void slimm_rf_lane_count(uint32_t* n, int why) {
    n[SLIMM_RF_N_JUDGED] += why != SLIMM_RF_NOT_JUDGED ? 1u : 0u;
    n[SLIMM_RF_N_FLAGS] += why == SLIMM_RF_FLAGS ? 1u : 0u;
    n[SLIMM_RF_N_MAPQ] += why == SLIMM_RF_MAPQ ? 1u : 0u;
    n[SLIMM_RF_N_ALIGNED] += why == SLIMM_RF_ALIGNED ? 1u : 0u;
    n[SLIMM_RF_N_IDENTITY] += (why == SLIMM_RF_IDENTITY || why == SLIMM_RF_NO_NM) ? 1u : 0u;
    n[SLIMM_RF_N_NO_NM] += why == SLIMM_RF_NO_NM ? 1u : 0u;
}
__device__ inline void slimm_rf_wave_add(uint32_t* counts, uint32_t* n) {
    if (!__any(static_cast<int>(n[SLIMM_RF_N_JUDGED]))) return;   /* (every other count is of judged records) */
    for (uint32_t k = 0; k <= SLIMM_RF_N_NO_NM; ++k) {
        uint32_t v = n[k];
        for (uint32_t d = 32u; d; d >>= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), static_cast<int>(d)));
        if (threadIdx.x == 0 && v) atomicAdd(&counts[k], v);
    }
}
#endif

/* one record's verdict into the counters (a host reader's; the device reduces over a wave first) */
SLIMM_RF_FN void slimm_rf_count(uint64_t* stats, int why) {
    if (why == SLIMM_RF_NOT_JUDGED) return;
    ++stats[SLIMM_RF_N_JUDGED];
    if (why == SLIMM_RF_FLAGS) ++stats[SLIMM_RF_N_FLAGS];
    if (why == SLIMM_RF_MAPQ) ++stats[SLIMM_RF_N_MAPQ];
    if (why == SLIMM_RF_ALIGNED) ++stats[SLIMM_RF_N_ALIGNED];
    if (why == SLIMM_RF_IDENTITY || why == SLIMM_RF_NO_NM) ++stats[SLIMM_RF_N_IDENTITY];
    if (why == SLIMM_RF_NO_NM) ++stats[SLIMM_RF_N_NO_NM];
}

/* slimm_host_record_passes_bam / _sam (include/slimm_hip.h), defined in the ONE translation unit that asks for them: the
 * library's context.hip -- and a stand-alone program that runs these very lines under a sanitizer
 * (tests/native/san_record_filter.cpp). */
#if defined(SLIMM_RF_HOST_API)
extern "C" int slimm_host_record_passes_bam(const slimm_record_filter* f, const uint8_t* record, uint32_t n_bytes, int* why) {
    if (!f || !record || !slimm_rf_valid(f)) return -1;
    const int verdict = slimm_rf_bam(f, record, n_bytes);
    if (why) *why = verdict;
    return slimm_rf_dropped(verdict) ? 0 : 1;
}
extern "C" int slimm_host_record_passes_sam(const slimm_record_filter* f, const char* line, uint32_t n_bytes, int* why) {
    if (!f || !line || !slimm_rf_valid(f)) return -1;
    const int verdict = slimm_rf_sam_line(f, (const uint8_t*)line, n_bytes);
    if (why) *why = verdict;
    return slimm_rf_dropped(verdict) ? 0 : 1;
}
#endif
