// The host xz decoder (slimm_amd/csrc/host/xz.cpp, xz_stream.h: the functions the device decoder runs too) as a stand-alone
// program, for the sanitizer pass (scripts/sanitize_host.sh) and the CPU tests (tests/test_xz_stream.py):
//   san_xz FILE...                  every file decoded: "FILE<tab>ok<tab>bytes<tab>crc64" or "FILE<tab>error<tab>message"
//   san_xz --out OUT FILE           the decoded bytes of FILE into OUT (exit 1 + the message on an error)
//   san_xz --counts FILE            what the decoder met: "name=value" lines (XzReader::Counts)
//   san_xz --index FILE             the blocks by the index reader: "stream<tab>at<tab>unpadded<tab>uncompressed" lines
//   san_xz --crc64 SEED N FILE      FILE's CRC64 from N random cuts, each piece from 0, folded: "ok" or "mismatch" per trial
//   san_xz --mutate SEED N FILE     N damaged copies of FILE decoded -- a byte flipped, the file cut short, a stretch of it
//                                   copied elsewhere --: "flips_same=a flips_differ=b others_ok=c errors=d"
//   san_xz --words SEED N FILE      the N damaged copies that `san_device_decoders xz FILE .. N SEED` makes (damaged_copies.h),
//                                   decoded: "trial T: ok" or "trial T: message" (tests/golden/codec_words)
// Damaged input must end in an error message, never in a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/host/xz.hpp"
#include "damaged_copies.h"

using slimm::XzReader;
namespace xz = slimm::xz;

static uint64_t crc64_step(uint64_t reg, const uint8_t* p, size_t n) {
    static uint64_t tab[256];
    static bool made = false;
    if (!made) {
        for (uint32_t i = 0; i < 256u; ++i) tab[i] = xz::crc64_table_entry(i);
        made = true;
    }
    for (size_t i = 0; i < n; ++i) reg = tab[(reg ^ p[i]) & 0xffu] ^ (reg >> 8);
    return reg;
}

using damage::rng;
using damage::slurp;

static bool decode(const std::vector<uint8_t>& blob, std::vector<uint8_t>* keep, uint64_t& n, uint64_t& crc, std::string& err, XzReader::Counts* counts) {
    size_t fed = 0;
    XzReader r([&](uint8_t* d, size_t cap) {
        const size_t k = std::min(cap, blob.size() - fed);
        if (k) memcpy(d, blob.data() + fed, k);
        fed += k;
        return k;
    });
    std::vector<uint8_t> buf(77777);   // (no multiple of a chunk's size: reads end inside chunks)
    long got;
    n = 0;
    uint64_t reg = ~0ull;
    while ((got = r.read(buf.data(), buf.size())) > 0) {
        reg = crc64_step(reg, buf.data(), static_cast<size_t>(got));
        if (keep) keep->insert(keep->end(), buf.begin(), buf.begin() + got);
        n += static_cast<uint64_t>(got);
    }
    crc = ~reg;
    if (got < 0) err = r.error();
    if (counts) *counts = r.counts();
    return got == 0;
}

int main(int argc, char** argv) {
    std::vector<uint8_t> blob;
    if (argc >= 3 && strcmp(argv[1], "--counts") == 0) {
        if (!slurp(argv[2], blob)) return 2;
        uint64_t n = 0, h = 0;
        std::string err;
        XzReader::Counts c;
        if (!decode(blob, nullptr, n, h, err, &c)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        const std::pair<const char*, uint64_t> rows[] = {{"streams", c.streams}, {"blocks", c.blocks}, {"lzma_chunks", c.lzma_chunks},
            {"raw_chunks", c.raw_chunks}, {"state_resets", c.state_resets}, {"prop_changes", c.prop_changes}, {"odd_props", c.odd_props},
            {"check_none", c.check_none}, {"check_crc32", c.check_crc32}, {"check_crc64", c.check_crc64}, {"sha256_unverified", c.sha256_unverified},
            {"match_bytes", c.match_bytes}, {"max_dist", c.max_dist}, {"text", c.text}, {"index_records", c.index_records}};
        for (const auto& r : rows) printf("%s=%llu\n", r.first, static_cast<unsigned long long>(r.second));
        return 0;
    }
    if (argc >= 3 && strcmp(argv[1], "--index") == 0) {
        if (!slurp(argv[2], blob)) return 2;
        std::vector<slimm::XzIndexBlock> blocks;
        uint32_t streams = 0;
        const bool ok = slimm::xz_read_index([&](uint64_t at, uint8_t* d, size_t n) {
            if (at > blob.size() || n > blob.size() - at) return false;
            memcpy(d, blob.data() + at, n);
            return true;
        }, blob.size(), &blocks, &streams);
        if (!ok) {
            printf("no index\n");
            return 1;
        }
        for (const auto& b : blocks)
            printf("%u\t%llu\t%llu\t%llu\n", b.stream, static_cast<unsigned long long>(b.at), static_cast<unsigned long long>(b.unpadded),
                   static_cast<unsigned long long>(b.uncompressed));
        return 0;
    }
    if (argc >= 5 && strcmp(argv[1], "--crc64") == 0) {
        damage::seed(strtoull(argv[2], nullptr, 10));
        const int trials = atoi(argv[3]);
        if (!slurp(argv[4], blob)) return 2;
        const uint64_t serial = crc64_step(~0ull, blob.data(), blob.size());
        for (int t = 0; t < trials; ++t) {
            uint64_t reg = ~0ull;
            for (size_t at = 0; at < blob.size();) {   // (pieces of 1 .. 5 000 bytes, each from 0: r * x^(8 n) + reg(0, piece))
                const size_t n = std::min<size_t>(blob.size() - at, 1u + rng() % 5000u);
                reg = xz::crc64_mul(reg, xz::crc64_x_pow8(n)) ^ crc64_step(0, blob.data() + at, n);
                at += n;
            }
            printf("%s\n", reg == serial ? "ok" : "mismatch");
        }
        printf("%016llx\n", static_cast<unsigned long long>(~serial));
        return 0;
    }
    if (argc >= 5 && strcmp(argv[1], "--mutate") == 0) {
        damage::seed(strtoull(argv[2], nullptr, 10));
        const int trials = atoi(argv[3]);
        if (!slurp(argv[4], blob) || blob.empty()) return 2;
        std::vector<uint8_t> good;
        uint64_t n0 = 0, h0 = 0, n = 0, h = 0;
        std::string err;
        if (!decode(blob, &good, n0, h0, err, nullptr)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        unsigned long long same = 0, differ = 0, others = 0, errors = 0;
        for (int t = 0; t < trials; ++t) {
            uint32_t kind = 0;
            const std::vector<uint8_t> b = damage::damaged(blob, false, 0, &kind);
            err.clear();
            const bool ok = decode(b, nullptr, n, h, err, nullptr);
            if (!ok && err.empty()) return 3;   // (an error without words)
            if (!ok) ++errors;
            else if (kind >= 2u) ++others;
            else if (n == n0 && h == h0) ++same;
            else
                ++differ;
        }
        printf("flips_same=%llu flips_differ=%llu others_ok=%llu errors=%llu\n", same, differ, others, errors);
        return 0;
    }
    if (argc >= 5 && strcmp(argv[1], "--words") == 0) {
        if (!slurp(argv[4], blob) || blob.empty()) return 2;
        damage::device_trials(blob, strtoull(argv[2], nullptr, 10), atoi(argv[3]), [](int t, const std::vector<uint8_t>& b) {
            uint64_t n = 0, h = 0;
            std::string err;
            printf("trial %d: %s\n", t, decode(b, nullptr, n, h, err, nullptr) ? "ok" : err.c_str());
        });
        return 0;
    }
    if (argc >= 4 && strcmp(argv[1], "--out") == 0) {
        if (!slurp(argv[3], blob)) return 2;
        std::vector<uint8_t> text;
        uint64_t n = 0, h = 0;
        std::string err;
        if (!decode(blob, &text, n, h, err, nullptr)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o || (!text.empty() && fwrite(text.data(), 1, text.size(), o) != text.size())) return 2;
        fclose(o);
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        blob.clear();
        uint64_t n = 0, h = 0;
        std::string err = "cannot open";
        if (slurp(argv[i], blob) && decode(blob, nullptr, n, h, err, nullptr))
            printf("%s\tok\t%llu\t%016llx\n", argv[i], static_cast<unsigned long long>(n), static_cast<unsigned long long>(h));
        else
            printf("%s\terror\t%s\n", argv[i], err.c_str());
    }
    return 0;
}
