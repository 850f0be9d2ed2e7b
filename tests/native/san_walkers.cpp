// TEST INFRASTRUCTURE ONLY -- the container walkers (slimm_amd/csrc/zstd_walk.h, xz_walk.h) as a stand-alone program under
// AddressSanitizer and UBSan; tests/test_codec_walkers.py builds and runs it.  What a walk finds must not depend on where the
// bytes are cut:
//   san_walkers XZ_FILE ZSTD_FILE [XZ_FILE_OF_MANY_BLOCKS]
// Per codec, over the good file and 200 damaged copies of it (damaged_copies.h, fixed seeds): the walker once over the whole
// buffer, then with the bytes arriving in pieces -- single bytes around every structural boundary of the good file, random
// pieces of 1 .. 5 000 bytes, the file in two halves.  The bytes at hand are always a heap copy of exactly their size, the
// next piece is appended at every "needs more bytes", and at the end the walker is told that the input is over.  Both runs
// must give the same items (kind, offset, sizes) and the same end (ended, or the same place and status).
// xz, also: every block start as the start of a range that was told the stream's check kind -- the index item must hand
// back exactly the records of the blocks in front of that start.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/xz_walk.h"
#include "../../slimm_amd/csrc/zstd_walk.h"
#include "damaged_copies.h"

using damage::Bytes;
namespace xz = slimm::xz;
namespace zs = slimm::zs;

// an item, or the walk's end, as a line
static std::string line(const zs::Walker::Item& it) {
    char b[200];
    snprintf(b, sizeof b, "%d %d@%llu st%u +%llu t%u s%u l%d c%08x", it.kind, static_cast<int>(it.place), static_cast<unsigned long long>(it.at), it.status,
             static_cast<unsigned long long>(it.bytes), it.type, it.size, it.last, it.sum);
    return b;
}
static std::string line(const xz::Walker::Item& it) {
    char b[240];
    snprintf(b, sizeof b, "%d %d@%llu st%u +%llu k%u h%u u%u c%u p%u r%llu/%llu n%llu i%llu kept%zu", it.kind, static_cast<int>(it.place),
             static_cast<unsigned long long>(it.at), it.status, static_cast<unsigned long long>(it.bytes), it.check, it.chunk.header, it.chunk.usize, it.chunk.csize,
             it.pad, static_cast<unsigned long long>(it.record.first), static_cast<unsigned long long>(it.record.second),
             static_cast<unsigned long long>(it.count), static_cast<unsigned long long>(it.index_bytes), it.kept.size());
    return b;
}

// The walk of `blob` with its bytes arriving at `cuts` (ascending offsets inside it; none: the whole buffer at once): every
// item as a line, the end as the last line.  What has been walked past is dropped, as both callers do
template <typename Walker>
static std::vector<std::string> walk(Walker w, const Bytes& blob, const std::vector<size_t>& cuts, std::vector<typename Walker::Item>* items = nullptr,
                                     size_t from = 0) {
    std::vector<std::string> out;
    size_t pos = from, fed = from, next_cut = 0;
    std::unique_ptr<uint8_t[]> have;   // blob[held_from, fed), exactly
    auto feed = [&]() {
        while (next_cut < cuts.size() && cuts[next_cut] <= fed) ++next_cut;
        const size_t to = next_cut < cuts.size() ? cuts[next_cut] : blob.size();
        if (to == fed) return false;
        fed = to;
        return true;
    };
    size_t held_from = 0, held_to = blob.size() + 1u;   // (nothing held yet)
    for (;;) {
        if (held_to != fed) {   // (its end is the end of what has come: a read past it is a report)
            have.reset(new uint8_t[fed - pos]);
            if (fed > pos) memcpy(have.get(), blob.data() + pos, fed - pos);
            held_from = pos, held_to = fed;
        }
        const typename Walker::Item it = w.peek(have.get() + (pos - held_from), fed - pos, pos);
        if ((it.kind == Walker::More || it.kind == Walker::MayEnd) && feed()) continue;
        if (it.kind <= Walker::MayEnd) {   // (the input is over: it ended, or the place and status of what is wrong or cut short)
            char b[100];
            snprintf(b, sizeof b, "end %d %d@%llu st%u", it.kind == Walker::MayEnd, static_cast<int>(it.place), static_cast<unsigned long long>(it.at), it.status);
            out.push_back(it.kind == Walker::MayEnd ? "ended" : b);
            return out;
        }
        out.push_back(line(it));
        if (items) items->push_back(it);
        w.take(it);
        pos += it.bytes;
    }
}

static std::vector<size_t> sorted_unique(std::vector<size_t> v, size_t size) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    while (!v.empty() && v.back() >= size) v.pop_back();
    while (!v.empty() && v.front() == 0) v.erase(v.begin());
    return v;
}

template <typename Walker>
static bool codec(const char* name, const Bytes& good, uint64_t seed, unsigned long long* n_items) {
    std::vector<typename Walker::Item> items;
    const std::vector<std::string> whole_good = walk(Walker(), good, {}, &items);
    if (whole_good.back() != "ended") {
        fprintf(stderr, "%s: the good file does not walk to its end: %s\n", name, whole_good.back().c_str());
        return false;
    }
    std::vector<size_t> bounds;   // single bytes around every structural boundary of the good file
    for (const auto& it : items)
        for (size_t k = 0; k < 7u; ++k)
            if (it.at + k >= 3u) bounds.push_back(static_cast<size_t>(it.at + k - 3u));
    damage::seed(seed);
    for (int copy = -1; copy < 200; ++copy) {
        const Bytes b = copy < 0 ? good : damage::damaged(good, false, 0);
        const std::vector<std::string> whole = walk(Walker(), b, {});
        *n_items += whole.size();
        const uint64_t keep = damage::rng_state;   // (the cuts draw from a seed of their own: the copies stay the same whatever the cuts)
        damage::seed(seed + 1000u);
        const std::vector<size_t> patterns[3] = {sorted_unique(bounds, b.size()), damage::random_cuts(b, false, 0), sorted_unique({b.size() / 2u}, b.size())};
        damage::rng_state = keep;
        for (int k = 0; k < 3; ++k) {
            const std::vector<std::string> pieces = walk(Walker(), b, patterns[k]);
            if (pieces == whole) continue;
            size_t d = 0;
            while (d < pieces.size() && d < whole.size() && pieces[d] == whole[d]) ++d;
            fprintf(stderr, "%s copy %d, pattern %d (%zu cuts): line %zu differs\n  whole:  %s\n  pieces: %s\n", name, copy, k, patterns[k].size(), d,
                    d < whole.size() ? whole[d].c_str() : "-", d < pieces.size() ? pieces[d].c_str() : "-");
            return false;
        }
    }
    return true;
}

// every block start as the start of a range that was told the check kind: what the stream's index hands back
static bool xz_kept(const char* path, const Bytes& blob, unsigned long long* n_starts) {
    std::vector<xz::Walker::Item> items;
    if (walk(xz::Walker(), blob, {}, &items).back() != "ended") {
        fprintf(stderr, "%s does not walk to its end\n", path);
        return false;
    }
    uint32_t check = 0;
    std::vector<xz::Walker::Record> in_front;
    for (size_t i = 0; i < items.size(); ++i) {
        if (items[i].kind == xz::Walker::StreamStart) check = items[i].check, in_front.clear();
        if (items[i].kind == xz::Walker::BlockEnd) in_front.push_back(items[i].record);
        if (items[i].kind != xz::Walker::BlockStart) continue;
        xz::Walker w;
        w.among_blocks(check);
        std::vector<xz::Walker::Item> mine;
        const std::vector<size_t> cuts = sorted_unique({static_cast<size_t>(items[i].at) + 1u, (static_cast<size_t>(items[i].at) + blob.size()) / 2u}, blob.size());
        walk(w, blob, cuts, &mine, static_cast<size_t>(items[i].at));
        const xz::Walker::Item* index = nullptr;
        for (const auto& it : mine)
            if (it.kind == xz::Walker::Index && !index) index = &it;
        if (!index || index->kept != in_front) {
            fprintf(stderr, "%s: a range from the block at byte %llu: the index keeps %zu records, %zu blocks lie in front\n", path,
                    static_cast<unsigned long long>(items[i].at), index ? index->kept.size() : 0u, in_front.size());
            return false;
        }
        ++*n_starts;
    }
    return true;
}

int main(int argc, char** argv) {
    Bytes x, z, many;
    if (argc < 3 || !damage::slurp(argv[1], x) || !damage::slurp(argv[2], z) || x.empty() || z.empty() || (argc > 3 && !damage::slurp(argv[3], many))) {
        fprintf(stderr, "usage: san_walkers XZ_FILE ZSTD_FILE [XZ_FILE_OF_MANY_BLOCKS]\n");
        return 2;
    }
    unsigned long long n_xz = 0, n_zs = 0, starts = 0;
    if (!codec<xz::Walker>("xz", x, 21, &n_xz) || !codec<zs::Walker>("zstd", z, 22, &n_zs)) return 1;
    if (!xz_kept(argv[1], x, &starts) || (argc > 3 && !xz_kept(argv[3], many, &starts))) return 1;
    printf("xz: 201 files, %llu items; zstd: 201 files, %llu items; %llu range starts: ok\n", n_xz, n_zs, starts);
    return 0;
}
