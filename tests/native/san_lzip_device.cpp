// TEST INFRASTRUCTURE ONLY -- the lzip device decoder's KERNELS (k_lzip_decode, and k_xz_check / k_xz_fold on its members) under
// AddressSanitizer and UBSan, on the CPU: san_device_decoders (its description holds here word for word) for a codec that
// program does not know, as san_lz4_device is for lz4.  This file and the emulator's
// objects (the product's .hip sources compiled by g++ with -fsanitize=address,undefined: `make -C tests/native
// san_device_decoders` builds them into emu_build_san) are one stand-alone program; tests/test_lzip_sanitized.py links and runs it.
//   san_lzip_device lzip FILE SKIP RECORDS TRIALS SEED
// FILE: a good lzip SAM input of RECORDS records whose references are R0 .. R3 (5 000 bases each), SKIP bytes of header in its
// decoded form.  The file is pushed whole and in pieces of 1 .. 5 000 bytes, every piece from a heap copy of exactly its size:
// both must give SLIMM_OK and RECORDS records.  Then TRIALS damaged copies (damaged_copies.h: the copies the other programs
// make of one SEED), slimm_reset between them: each must give SLIMM_OK or an error with words.  Prints "ok=a errors=b total=c".
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

struct Pusher {
    slimm_ctx* ctx;
    uint32_t skip;
    std::vector<std::unique_ptr<uint8_t[]>> held;

    int piece(const uint8_t* p, size_t n, bool first, bool last, uint64_t* got) {
        uint8_t* copy = nullptr;
        if (n) {   // (exactly n bytes on the heap: a read one byte past the input is a report)
            held.emplace_back(new uint8_t[n]);
            copy = held.back().get();
            memcpy(copy, p, n);
        }
        return slimm_push_lzip_sam_bytes(ctx, copy, n, first ? skip : 0u, last, got);
    }

    // The file at `cuts` (ascending offsets inside it)
    int file(const Bytes& blob, const std::vector<size_t>& cuts, uint64_t* records) {
        *records = 0;
        size_t at = 0;
        int rc = SLIMM_OK;
        for (size_t k = 0; k <= cuts.size() && rc == SLIMM_OK; ++k) {
            const size_t end = k < cuts.size() ? cuts[k] : blob.size();
            uint64_t got = 0;
            rc = piece(blob.data() + at, end - at, at == 0, k == cuts.size(), &got);
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

int main(int argc, char** argv) {
    if (argc != 7 || strcmp(argv[1], "lzip") != 0) {
        fprintf(stderr, "usage: san_lzip_device lzip FILE SKIP RECORDS TRIALS SEED\n");
        return 2;
    }
    Bytes blob;
    if (!slurp(argv[2], blob) || blob.empty()) {
        fprintf(stderr, "no such file\n");
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

    Pusher push{ctx, skip, {}};
    // the good file: whole, and in pieces
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t got = 0;
        const std::vector<size_t> cuts = pass ? damage::random_cuts(blob, false, 0) : std::vector<size_t>();
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
        const Bytes b = damage::damaged(blob, false, 0);
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
