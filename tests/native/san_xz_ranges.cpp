// The host functions by which an xz file is planned into byte ranges (slimm_amd/csrc/host/xz.cpp: xz_read_index,
// xz_plan_ranges, xz_check_at) as a stand-alone program for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wextra tests/native/san_xz_ranges.cpp slimm_amd/csrc/host/xz.cpp -o san_xz_ranges
//   san_xz_ranges tests/golden/xz/*.xz
// Every file is planned as it is -- 1 to 5 members and as many as it has bytes, with and without a header to skip, the check
// kind asked at every offset of the plan and at every 64th byte --, then truncated at every 4-byte step of its last 256
// bytes, and with 100 seeded single-bit flips in those bytes (the indexes and footers lie there).  Each copy lives in an
// allocation of exactly its size and is read without a bounds check of the program's own, so a read behind the bytes is a
// sanitizer report.  Damaged input must end in "no plan" or in offsets inside the file, never in a report.  Prints one
// line per file; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../slimm_amd/csrc/host/xz.hpp"

struct Counts {
    unsigned long long plans = 0, refused = 0, checks = 0;
};

// `n` bytes in an allocation of their own: the planner over them
static void feed(const uint8_t* bytes, size_t n, bool every_fourth, Counts& c) {
    std::unique_ptr<uint8_t[]> own(new uint8_t[n ? n : 1]);
    if (n) memcpy(own.get(), bytes, n);
    const uint8_t* p = own.get();
    const std::function<bool(uint64_t, uint8_t*, size_t)> read = [p](uint64_t off, uint8_t* dst, size_t k) {
        memcpy(dst, p + off, k);   // (no check here: the functions under test must stay inside `n`)
        return true;
    };
    for (uint64_t skip : {0ull, 1ull, 476ull, 1ull << 40}) {
        for (uint32_t members : {1u, 2u, 3u, 4u, 5u, static_cast<uint32_t>(n + 1u)}) {
            if (members > 5u && !every_fourth) continue;   // (as many members as bytes: the whole file only)
            std::vector<uint64_t> off(members + 1u, ~0ull);
            if (!slimm::xz_plan_ranges(read, n, skip, members, off.data())) {
                ++c.refused;
                continue;
            }
            ++c.plans;
            if (off[0] != 0 || off[members] != n) abort();
            for (uint32_t i = 0; i < members; ++i) {
                if (off[i] > off[i + 1]) abort();
                int kind = -2;
                if (members <= 5u && (!slimm::xz_check_at(read, n, off[i], &kind) || kind < -1 || kind > 15)) abort();
                ++c.checks;
            }
        }
    }
    for (size_t at = 0; every_fourth && at <= n; at += 64) {
        int kind = -2;
        if (slimm::xz_check_at(read, n, at, &kind) && (kind < -1 || kind > 15)) abort();
        ++c.checks;
    }
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> blob;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) blob.insert(blob.end(), buf, buf + got);
        fclose(f);
        Counts whole, cut, flips;
        feed(blob.data(), blob.size(), true, whole);
        const size_t tail = blob.size() < 256u ? blob.size() : 256u;
        for (size_t drop = 4; drop <= tail; drop += 4) feed(blob.data(), blob.size() - drop, false, cut);
        uint64_t seed = 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(i);
        for (int k = 0; k < 100 && tail; ++k) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const size_t bit = (blob.size() - tail) * 8u + static_cast<size_t>((seed >> 17) % (tail * 8u));
            blob[bit >> 3] ^= static_cast<uint8_t>(1u << (bit & 7u));
            feed(blob.data(), blob.size(), false, flips);
            blob[bit >> 3] ^= static_cast<uint8_t>(1u << (bit & 7u));
        }
        printf("%s\t%zu bytes\twhole: %llu plans, %llu refused, %llu checks\ttruncated: %llu plans, %llu refused\tflips: %llu plans, %llu refused\n", argv[i],
               blob.size(), whole.plans, whole.refused, whole.checks, cut.plans, cut.refused, flips.plans, flips.refused);
    }
    return 0;
}
