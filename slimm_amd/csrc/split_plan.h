// What the planners of split.hip (slimm_host_*_ranges) share: the regular file they read and its bounds-checked reader, the
// even shares their cuts start from, and the wrong cut that tests force.  Plain host C++ without the HIP runtime, so that
// tests/native/san_split_plan.cpp can run it under the sanitizers.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace slimm {

struct PlanFile {
    int fd = -1;
    uint64_t size = 0;
    ~PlanFile() {
        if (fd >= 0) ::close(fd);
    }
    // the size of a regular file, without opening it; false for anything else
    static bool regular_size(const char* path, uint64_t* size) {
        struct stat sb;
        if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
        *size = static_cast<uint64_t>(sb.st_size);
        return true;
    }
    // a regular file, opened for read(); asked before it is opened: opening a FIFO waits for its writer
    bool open_regular(const char* path) {
        struct stat sb;
        if (!regular_size(path, &size)) return false;
        fd = ::open(path, O_RDONLY);
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
        size = static_cast<uint64_t>(sb.st_size);
        return true;
    }
    bool read(uint64_t off, uint8_t* dst, size_t n) const {
        while (n) {
            const ssize_t k = pread(fd, dst, n, static_cast<off_t>(off));
            if (k <= 0) return false;
            dst += k;
            off += static_cast<uint64_t>(k);
            n -= static_cast<size_t>(k);
        }
        return true;
    }
    // the reader the container walks take (zstd_frame.h, xz_stream.h, gzip_plan.h): n bytes at off, false when they are not
    // all inside the file
    auto reader() const {
        return [this](uint64_t off, uint8_t* dst, size_t n) { return off <= size && n <= size - off && read(off, dst, n); };
    }
};

// The ranges of n members over a file of `size` bytes: offsets[0] = 0, offsets[n] = size, and offsets[i] in between is what
// `cut` makes of member i's even share of the bytes behind `floor` (no cut lies in front of it: member 0 holds the header).
// A cut that was not found (kNoCut) is the next one found, so the range in between is empty; the offsets never step back.
constexpr uint64_t kNoCut = ~0ull;
template <typename Cut>
void even_ranges(uint64_t floor, uint64_t size, uint32_t n, uint64_t* offsets, Cut cut) {
    offsets[0] = 0;
    offsets[n] = size;
    for (uint32_t i = 1; i < n; ++i) offsets[i] = cut(floor + static_cast<uint64_t>(static_cast<unsigned __int128>(size - floor) * i / n));
    for (uint32_t i = n; i-- > 1;)
        if (offsets[i] == kNoCut) offsets[i] = offsets[i + 1];
    for (uint32_t i = 1; i < n; ++i) offsets[i] = std::max(offsets[i], offsets[i - 1]);
}

// SLIMM_FORCE <codec>_split_wrong_cut: the second cut -- the first of two members -- lands one unit late, where nothing
// starts, and the cuts equal to it move with it (they are one cut): the members, or the stitch, must refuse it.  A cut at 0
// or at `limit` (the file's size in the offsets' unit, bytes or bits) or behind is no cut: the one in front of it is taken
inline void force_wrong_cut(uint64_t* offsets, uint32_t n, uint64_t limit) {
    if (n < 2) return;
    for (uint32_t i = std::min(2u, n - 1u); i >= 1u; --i) {
        const uint64_t was = offsets[i];
        if (was >= limit || was == 0) continue;
        for (uint32_t j = i; j < n && offsets[j] == was; ++j) ++offsets[j];
        break;
    }
}

}  // namespace slimm
