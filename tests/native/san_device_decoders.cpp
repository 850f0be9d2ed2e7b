// TEST INFRASTRUCTURE ONLY -- the device decoders' KERNELS under AddressSanitizer and UBSan, on the CPU: this file and the
// emulator's objects (the product's .hip sources compiled by g++ with -fsanitize=address,undefined: `make -C tests/native
// san_device_decoders`) are one stand-alone program.  The emulator's hipMalloc is one heap allocation per device buffer, so
// a kernel that reads or writes past a buffer on a damaged file ends here in a sanitizer report -- on a GPU it would be a
// fault, which no test may provoke.  tests/test_device_decoders_sanitized.py builds and runs it.
//   san_device_decoders CODEC FILE SKIP RECORDS TRIALS SEED
// CODEC: xz | zstd | gzip | bzip2 | bgzf_sam | bgzf_bam | sam.  FILE: a good input of RECORDS records whose references are
// R0 .. R3 (5 000 bases each), SKIP bytes of header in its decoded form.  The file is pushed whole and in pieces of
// 1 .. 5 000 bytes (BGZF: cut at the block boundaries behind them), every piece from a heap copy of exactly its size: both
// must give SLIMM_OK and RECORDS records.  Then TRIALS damaged copies -- a bit flipped, the file cut short, a stretch copied
// elsewhere; for `sam` damage to the text: a line cut, a tab removed, '@' at a line start --, slimm_reset between them: each
// must give SLIMM_OK or an error with words.  Prints "ok=a errors=b total=c" (and, with SAN_SHOW_WORDS set, every error's words).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "damaged_copies.h"
#include "slimm_hip.h"

using damage::Bytes;
using damage::slurp;

enum Codec { XZ, ZSTD, GZIP, BZIP2, BGZF_SAM, BGZF_BAM, SAM, N_CODECS };
static const char* const kCodecNames[N_CODECS] = {"xz", "zstd", "gzip", "bzip2", "bgzf_sam", "bgzf_bam", "sam"};

struct Pusher {
    slimm_ctx* ctx;
    Codec codec;
    uint32_t skip;
    // (the window forms read a buffer until the next call on the context has returned: the copies live as long as the file)
    std::vector<std::unique_ptr<uint8_t[]>> held;

    int piece(const uint8_t* p, size_t n, bool first, bool last, uint64_t* got) {
        uint8_t* copy = nullptr;
        if (n) {   // (exactly n bytes on the heap: a read one byte past the input is a report)
            held.emplace_back(new uint8_t[n]);
            copy = held.back().get();
            memcpy(copy, p, n);
        }
        const uint32_t sk = first ? skip : 0u;
        switch (codec) {
            case XZ: return slimm_push_xz_sam_bytes(ctx, copy, n, sk, last, got);
            case ZSTD: return slimm_push_zstd_sam_bytes(ctx, copy, n, sk, last, got);
            case GZIP: return slimm_push_gzip_sam_bytes(ctx, copy, n, sk, last, got);
            case BZIP2: return slimm_push_bzip2_sam_bytes(ctx, copy, n, sk, last, got);
            case BGZF_SAM: return slimm_push_bgzf_sam_blocks(ctx, copy, n, sk, last, got);
            case BGZF_BAM: return slimm_push_bgzf_blocks(ctx, copy, n, sk, last, got);
            default: return slimm_push_sam_bytes(ctx, copy, n, last, got);
        }
    }

    // The file at `cuts` (ascending offsets inside it); for `sam` the text behind its header.
    int file(const Bytes& blob, const std::vector<size_t>& cuts, uint64_t* records) {
        const size_t from = codec == SAM ? std::min<size_t>(skip, blob.size()) : 0u;
        *records = 0;
        size_t at = from;
        int rc = SLIMM_OK;
        for (size_t k = 0; k <= cuts.size() && rc == SLIMM_OK; ++k) {
            const size_t end = k < cuts.size() ? cuts[k] : blob.size();
            uint64_t got = 0;
            rc = piece(blob.data() + at, end - at, at == from, k == cuts.size(), &got);
            *records += got;
            at = end;
        }
        return rc;
    }

    void forget() {
        slimm_reset(ctx);
        held.clear();
    }
};

static std::vector<size_t> random_cuts(const Bytes& blob, Codec codec, size_t from) {
    return damage::random_cuts(blob, codec == BGZF_SAM || codec == BGZF_BAM, from);
}
static Bytes damaged(const Bytes& blob, Codec codec, size_t skip) { return damage::damaged(blob, codec == SAM, skip); }

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: san_device_decoders CODEC FILE SKIP RECORDS TRIALS SEED\n");
        return 2;
    }
    int codec = 0;
    while (codec < N_CODECS && strcmp(argv[1], kCodecNames[codec]) != 0) ++codec;
    Bytes blob;
    if (codec == N_CODECS || !slurp(argv[2], blob) || blob.empty()) {
        fprintf(stderr, "unknown codec, or no such file\n");
        return 2;
    }
    const uint32_t skip = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    const uint64_t records = strtoull(argv[4], nullptr, 10);
    const int trials = atoi(argv[5]);
    damage::seed(strtoull(argv[6], nullptr, 10));

    // four references of 5 000 bases, each a strain of its own species under shared higher ranks
    const uint32_t ref_len[4] = {5000, 5000, 5000, 5000};
    uint32_t lineage[4 * 8], tax_id[4 * 2 + 6], tax_rank[4 * 2 + 6];
    const char* tax_name[4 * 2 + 6];
    uint32_t n_taxa = 0;
    for (uint32_t r = 0; r < 4u; ++r) {
        lineage[r * 8u] = 1000u + r, lineage[r * 8u + 1u] = 100u + r;
        for (uint32_t k = 2; k < 8u; ++k) lineage[r * 8u + k] = 10u + k;
        tax_id[n_taxa] = 1000u + r, tax_rank[n_taxa] = SLIMM_RANK_STRAIN, tax_name[n_taxa++] = "a strain";
        tax_id[n_taxa] = 100u + r, tax_rank[n_taxa] = SLIMM_RANK_SPECIES, tax_name[n_taxa++] = "a species";
    }
    for (uint32_t k = 2; k < 8u; ++k) tax_id[n_taxa] = 10u + k, tax_rank[n_taxa] = k, tax_name[n_taxa++] = "a higher rank";
    slimm_config cfg{};
    cfg.n_refs = 4, cfg.ref_len = ref_len, cfg.lineage = lineage, cfg.bin_width = 0, cfg.avg_read_len = 150, cfg.min_reads = 0;
    cfg.cov_cut_off = 0.95f, cfg.abundance_cut_off = 0.01f, cfg.rank = "species";
    cfg.n_taxa = n_taxa, cfg.tax_id = tax_id, cfg.tax_rank = tax_rank, cfg.tax_name = tax_name;
    cfg.device = 0, cfg.record_order = SLIMM_ORDER_ANY;
    slimm_ctx* ctx = nullptr;
    if (slimm_create(&cfg, &ctx) != SLIMM_OK) {
        fprintf(stderr, "slimm_create: %s\n", slimm_last_error(nullptr));
        return 1;
    }
    const char* const names[4] = {"R0", "R1", "R2", "R3"};
    if (slimm_set_reference_names(ctx, names) != SLIMM_OK) return 1;

    Pusher push{ctx, static_cast<Codec>(codec), skip, {}};
    // the good file: whole, and in pieces
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t got = 0;
        const std::vector<size_t> cuts = pass ? random_cuts(blob, push.codec, codec == SAM ? skip : 0u) : std::vector<size_t>();
        const int rc = push.file(blob, cuts, &got);
        if (rc != SLIMM_OK || got != records) {
            fprintf(stderr, "the good file in %zu pieces: rc %d, %llu records of %llu: %s\n", cuts.size() + 1u, rc, static_cast<unsigned long long>(got),
                    static_cast<unsigned long long>(records), slimm_last_error(ctx));
            return 1;
        }
        push.forget();
    }
    unsigned long long ok = 0, errors = 0;
    const bool show_words = getenv("SAN_SHOW_WORDS") != nullptr;   // (for whoever reads a tally: what each damaged copy was refused with)
    for (int t = 0; t < trials; ++t) {
        const Bytes b = damaged(blob, push.codec, codec == SAM ? skip : 0u);
        uint64_t got = 0;
        const int rc = push.file(b, {}, &got);
        if (rc == SLIMM_OK) {
            ++ok;
        } else {
            const char* words = slimm_last_error(ctx);
            if (!words || !*words) {
                fprintf(stderr, "trial %d: rc %d without words\n", t, rc);
                return 3;
            }
            if (show_words) fprintf(stderr, "trial %d: %s\n", t, words);
            ++errors;
        }
        push.forget();
    }
    slimm_destroy(ctx);
    printf("ok=%llu errors=%llu total=%llu\n", ok, errors, ok + errors);
    return 0;
}
