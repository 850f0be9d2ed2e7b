// TEST INFRASTRUCTURE ONLY -- the one generator of damaged copies and of piece cuts that the sanitizer programs share
// (san_device_decoders, san_xz, san_zstd, san_walkers): the same SEED gives every program the same copies, so what the
// device decoders and the host readers say of one damaged file can be held side by side (tests/golden/codec_words).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace damage {

using Bytes = std::vector<uint8_t>;

inline uint64_t rng_state = 1;
inline void seed(uint64_t s) { rng_state = s * 2u + 1u; }
inline uint64_t rng() {   // (xorshift64*)
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

inline bool slurp(const char* path, Bytes& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

// Offsets 1 .. 5 000 bytes apart, from `from` on; bgzf: each moved up to the next block boundary of the (good) file.
inline std::vector<size_t> random_cuts(const Bytes& blob, bool bgzf, size_t from) {
    std::vector<size_t> ends;
    if (bgzf)
        for (size_t p = 0; p + 18u <= blob.size();) {
            p += (blob[p + 16] | (static_cast<size_t>(blob[p + 17]) << 8)) + 1u;
            ends.push_back(p);
        }
    std::vector<size_t> cuts;
    size_t at = from, e = 0;
    while (true) {
        at += 1u + rng() % 5000u;
        if (!ends.empty()) {
            while (e < ends.size() && ends[e] < at) ++e;
            if (e == ends.size()) break;
            at = ends[e];
        }
        if (at >= blob.size()) break;
        cuts.push_back(at);
    }
    return cuts;
}

// A damaged copy: a bit flipped (kinds 0, 1), the file cut short (2), a stretch copied elsewhere (3); text: also, somewhere
// behind the `skip` bytes of header, a line cut (4), the next tab removed (5), '@' at the next line's start (6).
inline Bytes damaged(const Bytes& blob, bool text, size_t skip, uint32_t* kind_out = nullptr) {
    Bytes b = blob;
    const uint32_t kind = static_cast<uint32_t>(rng() % (text ? 7u : 4u));
    if (kind_out) *kind_out = kind;
    if (kind < 2u) {
        b[rng() % b.size()] ^= static_cast<uint8_t>(1u << (rng() % 8u));
    } else if (kind == 2u) {
        b.resize(rng() % b.size());
    } else if (kind == 3u) {
        const size_t len = 1u + rng() % std::min<size_t>(b.size(), 4096u), from = rng() % (b.size() - len + 1u), to = rng() % (b.size() - len + 1u);
        memmove(b.data() + to, b.data() + from, len);
    } else {
        size_t at = skip + rng() % (b.size() - skip);
        const uint8_t want = kind == 5u ? '\t' : '\n';
        while (at < b.size() && b[at] != want) ++at;
        if (at + 1u >= b.size()) return b;
        if (kind == 4u) {
            const size_t k = std::min<size_t>(at - skip, 1u + rng() % 40u);
            b.erase(b.begin() + (at - k), b.begin() + at);
        }
        else if (kind == 5u) b.erase(b.begin() + static_cast<long>(at));
        else b[at + 1u] = '@';
    }
    return b;
}

// What san_device_decoders does with SEED in front of its trials (the good file once in random pieces), then its `trials`
// damaged copies: f(t, copy) for each.  The host programs' --words mode runs their reader over exactly those.
template <typename F>
inline void device_trials(const Bytes& blob, uint64_t seed_arg, int trials, F&& f) {
    seed(seed_arg);
    (void)random_cuts(blob, false, 0);
    for (int t = 0; t < trials; ++t) f(t, damaged(blob, false, 0));
}

}  // namespace damage
