// The host functions by which a zstd file is planned into byte ranges (slimm_amd/csrc/zstd_frame.h: cut_candidate,
// walk_blocks, frame_may_start; host/zstd.cpp: zstd_header_end) as a stand-alone program for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wextra tests/native/san_zstd_ranges.cpp slimm_amd/csrc/host/zstd.cpp -o san_zstd_ranges
//   san_zstd_ranges tests/golden/zstd_frames/*.zst tests/golden/zstd/*.zst
// Every file is fed as it is -- the candidate test at every byte, the chain walk behind every frame header --, the first two
// also cut to every prefix length, and every file with 2 000 seeded single-bit flips (the header's frames are decoded for
// the whole file, every 997th prefix and every 8th flip).  Each copy lives in an allocation of
// exactly its size and is read without a bounds check of the program's own, so a read behind the bytes is a sanitizer
// report.  Damaged input must end in "no cut", never in a report.  Prints one line per file; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/host/zstd.hpp"

namespace zs = slimm::zs;

struct Counts {
    unsigned long long candidates = 0, cuts = 0, walks = 0, chains = 0, headers = 0;
};

// `n` bytes in an allocation of their own: the planner's scan over them
static void feed(const uint8_t* bytes, size_t n, bool every_byte, bool header, Counts& c) {
    std::unique_ptr<uint8_t[]> own(new uint8_t[n ? n : 1]);
    if (n) memcpy(own.get(), bytes, n);
    const uint8_t* p = own.get();
    auto read = [p](uint64_t off, uint8_t* dst, size_t k) {
        memcpy(dst, p + off, k);   // (no check here: the functions under test must stay inside `n`)
        return true;
    };
    for (size_t at = 0; at < n; ++at) {
        const bool magic_byte = p[at] == 0x28u || (p[at] & 0xf0u) == 0x50u;
        if (!every_byte && !magic_byte) continue;
        uint64_t end = 0;
        ++c.candidates;
        if (zs::cut_candidate(read, n, at, &end)) {
            ++c.cuts;
            if (end > n || end <= at) abort();
        }
        if (n - at >= 4u && zs::le32(p + at) == zs::kMagic) {   // the chain behind whatever header stands here
            zs::FrameHeader fh;
            if (zs::frame_header(p + at, n - at, fh) == zs::kOk) {
                ++c.walks;
                if (zs::walk_blocks(read, n, at + fh.bytes, fh.block_max, fh.has_checksum, &end)) {
                    ++c.chains;
                    if (end > n) abort();
                }
            }
        }
    }
    (void)zs::frame_may_start(read, n, n);
    if (!header) return;   // (the header's frames are decoded: not for every prefix)
    for (uint64_t skip : {1ull, 476ull}) {
        uint64_t first = 0;
        const std::function<bool(uint64_t, uint8_t*, size_t)> r = read;
        if (slimm::zstd_header_end(r, n, skip, &first)) {
            ++c.headers;
            if (first > n) abort();
        }
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
        Counts whole, prefixes, flips;
        feed(blob.data(), blob.size(), true, true, whole);
        if (i <= 2)
            for (size_t n = 0; n < blob.size(); ++n) feed(blob.data(), n, false, n % 997u == 0, prefixes);
        uint64_t seed = 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(i);
        for (int k = 0; k < 2000; ++k) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const size_t bit = static_cast<size_t>((seed >> 17) % (blob.size() * 8u));
            blob[bit >> 3] ^= static_cast<uint8_t>(1u << (bit & 7u));
            feed(blob.data(), blob.size(), false, k % 8 == 0, flips);
            blob[bit >> 3] ^= static_cast<uint8_t>(1u << (bit & 7u));
        }
        printf("%s\t%zu bytes\twhole: %llu cuts of %llu candidates, %llu chains of %llu walks\tprefixes: %llu cuts of %llu\tflips: %llu cuts of %llu, %llu headers\n",
               argv[i], blob.size(), whole.cuts, whole.candidates, whole.chains, whole.walks, prefixes.cuts, prefixes.candidates, flips.cuts,
               flips.candidates, flips.headers);
    }
    return 0;
}
