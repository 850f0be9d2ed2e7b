// The host zstd decoder (slimm_amd/csrc/host/zstd.cpp, zstd_frame.h) as a stand-alone program, for the sanitizer pass
// (scripts/sanitize_host.sh) and the CPU tests (tests/test_zstd_frame.py):
//   san_zstd FILE...              every file decoded: "FILE<tab>ok<tab>bytes<tab>xxh64" or "FILE<tab>error<tab>message"
//   san_zstd --out OUT FILE       the decoded bytes of FILE into OUT (exit 1 + the message on an error)
//   san_zstd --xxh64 PIECE FILE   XXH64 of FILE's bytes, taken PIECE bytes at a time
//   san_zstd --words SEED N FILE  the N damaged copies that `san_device_decoders zstd FILE .. N SEED` makes (damaged_copies.h),
//                                 decoded: "trial T: ok" or "trial T: message" (tests/golden/codec_words)
// Damaged input must end in an error message, never in a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/host/zstd.hpp"
#include "damaged_copies.h"

static bool decode(const char* path, std::vector<uint8_t>* keep, uint64_t& n, uint64_t& hash, std::string& err) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        err = "cannot open";
        return false;
    }
    slimm::ZstdReader r([f](uint8_t* d, size_t cap) { return fread(d, 1, cap, f); });
    slimm::zs::Xxh64 x;
    x.reset();
    std::vector<uint8_t> buf(777777);   // (no multiple of a block's size: reads end inside blocks)
    long got;
    n = 0;
    while ((got = r.read(buf.data(), buf.size())) > 0) {
        x.update(buf.data(), static_cast<uint64_t>(got));
        if (keep) keep->insert(keep->end(), buf.begin(), buf.begin() + got);
        n += static_cast<uint64_t>(got);
    }
    fclose(f);
    hash = x.digest();
    if (got < 0) err = r.error();
    return got == 0;
}

int main(int argc, char** argv) {
    if (argc >= 5 && strcmp(argv[1], "--words") == 0) {
        std::vector<uint8_t> blob;
        if (!damage::slurp(argv[4], blob) || blob.empty()) return 2;
        damage::device_trials(blob, strtoull(argv[2], nullptr, 10), atoi(argv[3]), [](int t, const std::vector<uint8_t>& b) {
            size_t fed = 0;
            slimm::ZstdReader r([&](uint8_t* d, size_t cap) {
                const size_t k = std::min(cap, b.size() - fed);
                if (k) memcpy(d, b.data() + fed, k);
                fed += k;
                return k;
            });
            std::vector<uint8_t> buf(777777);
            long got;
            while ((got = r.read(buf.data(), buf.size())) > 0) {
            }
            printf("trial %d: %s\n", t, got == 0 ? "ok" : r.error().c_str());
        });
        return 0;
    }
    if (argc >= 4 && strcmp(argv[1], "--xxh64") == 0) {
        FILE* f = fopen(argv[3], "rb");
        if (!f) return 2;
        std::vector<uint8_t> piece(static_cast<size_t>(std::max(1, atoi(argv[2]))));
        slimm::zs::Xxh64 x;
        x.reset();
        size_t got;
        while ((got = fread(piece.data(), 1, piece.size(), f)) > 0) x.update(piece.data(), got);
        fclose(f);
        printf("%016llx\n", static_cast<unsigned long long>(x.digest()));
        return 0;
    }
    if (argc >= 4 && strcmp(argv[1], "--out") == 0) {
        std::vector<uint8_t> text;
        uint64_t n = 0, h = 0;
        std::string err;
        if (!decode(argv[3], &text, n, h, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o || (!text.empty() && fwrite(text.data(), 1, text.size(), o) != text.size())) return 2;
        fclose(o);
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        uint64_t n = 0, h = 0;
        std::string err;
        if (decode(argv[i], nullptr, n, h, err)) printf("%s\tok\t%llu\t%016llx\n", argv[i], static_cast<unsigned long long>(n), static_cast<unsigned long long>(h));
        else
            printf("%s\terror\t%s\n", argv[i], err.c_str());
    }
    return 0;
}
