// The planner of slimm_host_gzip_ranges (slimm_amd/csrc/gzip_plan.h on deflate_stream.h: plain host C++) as a stand-alone
// program for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wextra tests/native/san_gzip_plan.cpp -o san_gzip_plan
//   san_gzip_plan FILE.gz ...
// Each file is planned from a heap copy of exactly its size -- a read past it is a report -- for 2, 4 and 8 members with a
// skip of 0 and of 300; then every prefix of it in 64 steps, and 200 copies with a flipped bit each (a fixed seed).  A plan
// that is made starts at 0, ends at 8 x the size and never steps back; damage ends in "not planned" or in other cuts.
// Prints one line per file: "FILE: whole: <the 5 offsets for 4 members, skip 0>; <plans> plans, <refused> refused"; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../slimm_amd/csrc/gzip_plan.h"

static unsigned long long g_plans = 0, g_refused = 0;

static bool plan(const uint8_t* data, uint64_t size, uint64_t skip, uint32_t n, uint64_t* out) {
    auto read = [&](uint64_t off, uint8_t* dst, size_t k) {
        if (off > size || k > size - off) return false;
        memcpy(dst, data + off, k);
        return true;
    };
    slimm::GzipPlan knobs;
    knobs.cut_search = 1u << 20;
    if (!slimm::gzip_plan_ranges(read, size, skip, n, out, knobs)) {
        ++g_refused;
        return false;
    }
    if (out[0] != 0 || out[n] != size * 8u) abort();
    for (uint32_t i = 0; i < n; ++i)
        if (out[i] > out[i + 1]) abort();
    ++g_plans;
    return true;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> all;
        uint8_t tmp[4096];
        for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) all.insert(all.end(), tmp, tmp + k);
        fclose(f);
        g_plans = g_refused = 0;
        uint64_t whole[5] = {};
        for (uint32_t n : {2u, 4u, 8u})
            for (uint64_t skip : {uint64_t(0), uint64_t(300)}) {
                std::unique_ptr<uint8_t[]> copy(new uint8_t[all.size()]);
                memcpy(copy.get(), all.data(), all.size());
                std::unique_ptr<uint64_t[]> out(new uint64_t[n + 1u]);
                if (plan(copy.get(), all.size(), skip, n, out.get()) && n == 4u && skip == 0) memcpy(whole, out.get(), sizeof whole);
            }
        for (uint64_t step = 1; step <= 64; ++step) {   // prefixes: the file ends anywhere
            const size_t size = all.size() * step / 65u;
            std::unique_ptr<uint8_t[]> copy(new uint8_t[size ? size : 1u]);
            memcpy(copy.get(), all.data(), size);
            uint64_t out[4];
            (void)plan(copy.get(), size, step % 2u ? 300u : 0u, 3, out);
        }
        uint64_t seed = 0x9e3779b97f4a7c15ull;
        for (int t = 0; t < 200; ++t) {   // flipped bits
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            std::unique_ptr<uint8_t[]> copy(new uint8_t[all.size()]);
            memcpy(copy.get(), all.data(), all.size());
            if (!all.empty()) copy[(seed >> 20) % all.size()] ^= static_cast<uint8_t>(1u << ((seed >> 8) & 7u));
            uint64_t out[5];
            (void)plan(copy.get(), all.size(), t % 2 ? 300u : 0u, 4, out);
        }
        printf("%s: whole: %llu %llu %llu %llu %llu; %llu plans, %llu refused\n", argv[a], (unsigned long long)whole[0], (unsigned long long)whole[1],
               (unsigned long long)whole[2], (unsigned long long)whole[3], (unsigned long long)whole[4], g_plans, g_refused);
    }
    return 0;
}
