// What the range planners of slimm_amd/csrc/split.hip share (slimm_amd/csrc/split_plan.h: PlanFile, even_ranges, force_wrong_cut) as a
// stand-alone program for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wextra tests/native/san_split_plan.cpp -o san_split_plan
//   san_split_plan WORKDIR
// even_ranges over sizes, floors and member counts (0 and 1 bytes, floor = size, sizes near 2^64) with cuts that are exact,
// searched forward, not found, or all not found, into an allocation of exactly n + 1 offsets: the offsets start at 0, end at
// the size and never step back.  PlanFile on a file it writes under WORKDIR, a directory, a FIFO (which must be refused
// without being opened: opening it would wait for a writer) and a missing path; its reader inside and across the file's end.
// force_wrong_cut on allocations of exactly n + 1 offsets: one member, cuts at the limit, equal cuts, a cut at 0.  Prints one
// line; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../slimm_amd/csrc/split_plan.h"

using slimm::kNoCut;

static unsigned long long g_plans = 0;

template <typename Cut>
static void plan(uint64_t floor, uint64_t size, uint32_t n, Cut cut) {
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1u]);
    slimm::even_ranges(floor, size, n, off.get(), cut);
    if (off[0] != 0 || off[n] != size) abort();
    for (uint32_t i = 0; i < n; ++i)
        if (off[i] > off[i + 1]) abort();
    ++g_plans;
}

// force_wrong_cut over `in` (n + 1 offsets, the last one the limit) gives `want`
static void wrong_cut(std::initializer_list<uint64_t> in, std::initializer_list<uint64_t> want) {
    const uint32_t n = static_cast<uint32_t>(in.size()) - 1u;
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1u]);
    std::copy(in.begin(), in.end(), off.get());
    slimm::force_wrong_cut(off.get(), n, off[n]);
    if (!std::equal(want.begin(), want.end(), off.get())) abort();
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const uint64_t sizes[] = {0, 1, 2, 17, 4096, (1ull << 32) + 5, ~0ull - 1};
    for (uint64_t size : sizes)
        for (uint64_t floor : {uint64_t(0), size / 3, size})
            for (uint32_t n : {1u, 2u, 3u, 7u, 128u}) {
                plan(floor, size, n, [](uint64_t t) { return t; });
                plan(floor, size, n, [&](uint64_t t) { return std::min(size, t | 0xfffu); });            // (the next "block start")
                plan(floor, size, n, [&](uint64_t t) { return (t / 3u) % 2u ? kNoCut : t; });            // (some searches give up)
                plan(floor, size, n, [](uint64_t) { return kNoCut; });                                   // (a file of one frame)
            }
    wrong_cut({0, 100}, {0, 100});                                    // n = 1 changes nothing
    wrong_cut({0, 100, 100, 100}, {0, 100, 100, 100});                // cuts that all equal the limit are unchanged
    wrong_cut({0, 40, 70, 70, 70, 100}, {0, 40, 71, 71, 71, 100});    // equal neighbouring cuts move together by one
    wrong_cut({0, 40, 70, 100}, {0, 40, 71, 100});                    // (the second cut, where there are two)
    wrong_cut({0, 40, 100}, {0, 41, 100});                            // (of two members: their only one)
    wrong_cut({0, 0, 100}, {0, 0, 100});                              // a cut at 0 is skipped
    wrong_cut({0, 40, 100, 100}, {0, 41, 100, 100});                  // (the second cut at the limit: the first is taken)
    wrong_cut({0, 0, 0, 100}, {0, 0, 0, 100});
    const std::string dir = argv[1], file = dir + "/plan_file", fifo = dir + "/plan_fifo";
    {
        FILE* f = fopen(file.c_str(), "wb");
        if (!f || fwrite("0123456789", 1, 10, f) != 10 || fclose(f) != 0) return 2;
        slimm::PlanFile p;
        uint8_t got[10] = {};
        if (!p.open_regular(file.c_str()) || p.size != 10 || !p.read(3, got, 7) || memcmp(got, "3456789", 7) != 0) abort();
        if (p.read(5, got, 6)) abort();   // (behind the file's end: a short read is a failure, not a loop)
        const auto read = p.reader();     // (the same, refused before it is tried)
        if (!read(3, got, 7) || memcmp(got, "3456789", 7) != 0 || !read(10, got, 0) || read(5, got, 6) || read(11, got, 0) || read(~0ull, got, 2)) abort();
        uint64_t size = 0;
        if (!slimm::PlanFile::regular_size(file.c_str(), &size) || size != 10) abort();
    }
    (void)remove(fifo.c_str());
    if (mkfifo(fifo.c_str(), 0600) != 0) return 2;
    for (const std::string& path : {dir, fifo, dir + "/no_such_file"}) {
        slimm::PlanFile p;
        uint64_t size = 0;
        if (p.open_regular(path.c_str()) || p.fd >= 0 || slimm::PlanFile::regular_size(path.c_str(), &size)) abort();
    }
    (void)remove(fifo.c_str());
    (void)remove(file.c_str());
    printf("san_split_plan: %llu plans, 8 wrong cuts, 4 paths: ok\n", g_plans);
    return 0;
}
