// The host lzip decoder and the member finder (slimm_amd/csrc/host/lzip.cpp, lzip_member.h, lzip_walk.h) as a stand-alone
// program, for the sanitizer pass and the CPU tests (tests/test_lzip_member.py, tests/test_lzip_sanitized.py):
//   san_lzip FILE...              every file decoded: "FILE<tab>ok<tab>bytes<tab>crc32<tab>members empty match_bytes max_dist
//                                 max_dict" or "FILE<tab>error<tab>message"
//   san_lzip --out OUT FILE       the decoded bytes of FILE into OUT (exit 1 + the message on an error)
//   san_lzip --members OUT FILE   every member's text into OUT.<k> (exit 1 + the message on an error)
//   san_lzip --walk FILE          the members by lzip::Walker over the whole file, one a line: "member AT SIZE DICT DATA_SIZE CRC",
//                                 and "error <words>" where it stops
//   san_lzip --feed STEP FILE     the same lines, the walker fed STEP more bytes a peek (its cursor kept), then "peeks N searched M":
//                                 M = the bytes the searches looked at in all
//   san_lzip --index FILE         the members by lzip_read_index, from the file's end: "member AT SIZE DATA_SIZE", or "error"
//   san_lzip --damage SEED N FILE N damaged copies of FILE (damaged_copies.h) and every truncation of its first 300 bytes,
//                                 decoded, walked and indexed: "ok=a errors=b total=c"
// Damaged input must end in an error message, never in a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/host/lzip.hpp"
#include "damaged_copies.h"

using slimm::lzip::Walker;

static bool decode(const std::vector<uint8_t>& b, std::vector<uint8_t>* keep, uint64_t& n, uint32_t& crc, std::string& err, slimm::LzipReader::Counts* counts) {
    size_t fed = 0;
    slimm::LzipReader r([&](uint8_t* d, size_t cap) {
        const size_t k = std::min(cap, b.size() - fed);
        if (k) memcpy(d, b.data() + fed, k);
        fed += k;
        return k;
    });
    std::vector<uint8_t> buf(77777);   // (reads end inside members)
    long got;
    n = 0;
    uint32_t c = 0xffffffffu;
    while ((got = r.read(buf.data(), buf.size())) > 0) {
        for (long i = 0; i < got; ++i) c = slimm::gz::crc_table_entry((c ^ buf[static_cast<size_t>(i)]) & 0xffu) ^ (c >> 8);
        if (keep) keep->insert(keep->end(), buf.begin(), buf.begin() + got);
        n += static_cast<uint64_t>(got);
    }
    crc = ~c;
    if (got < 0) err = r.error();
    if (counts) *counts = r.counts();
    return got == 0;
}

// the walker over b, fed `step` more bytes a peek (0: all at once); `out`: where the lines go (null: nowhere)
static bool walk(const std::vector<uint8_t>& b, size_t step, FILE* out) {
    Walker w;
    uint64_t pos = 0, peeks = 0, looked = 0;
    size_t have = step ? std::min(step, b.size()) : b.size();
    bool good = true;
    for (;;) {
        const bool at_end = have == b.size();
        const Walker::Item it = w.peek(b.data() + pos, have - pos, pos, at_end);
        ++peeks;
        if (it.kind == Walker::MayEnd) {
            if (at_end) break;
            have = std::min(b.size(), have + step);
            continue;
        }
        if (it.kind == Walker::More && !at_end) {
            looked += it.searched > std::max(w.searched, pos) ? it.searched - std::max(w.searched, pos) : 0u;
            w.take(it);
            have = std::min(b.size(), have + step);
            continue;
        }
        if (it.kind == Walker::More || it.kind == Walker::Error) {
            if (out) fprintf(out, "error %s\n", it.words().c_str());
            good = false;
            break;
        }
        if (out)
            fprintf(out, "member %llu %llu %u %llu %08x\n", (unsigned long long)it.at, (unsigned long long)it.bytes, it.dict_size,
                    (unsigned long long)it.trailer.data_size, it.trailer.crc);
        looked += pos + it.bytes - std::max(w.searched, pos);
        w.take(it);
        pos += it.bytes;
    }
    if (out && step) fprintf(out, "peeks %llu searched %llu\n", (unsigned long long)peeks, (unsigned long long)looked);
    return good;
}

static bool index(const std::vector<uint8_t>& b, FILE* out) {
    std::vector<slimm::LzipIndexMember> members;
    const bool ok = slimm::lzip_read_index(
        [&](uint64_t at, uint8_t* dst, size_t n) {
            if (at > b.size() || n > b.size() - at) return false;
            if (n) memcpy(dst, b.data() + at, n);
            return true;
        },
        b.size(), &members);
    if (!out) return ok;
    if (!ok) fprintf(out, "error\n");
    else
        for (const slimm::LzipIndexMember& m : members)
            fprintf(out, "member %llu %llu %llu\n", (unsigned long long)m.at, (unsigned long long)m.member_size, (unsigned long long)m.data_size);
    return ok;
}

int main(int argc, char** argv) {
    std::vector<uint8_t> blob;
    if (slimm::lzip::kProbs != slimm::xz::n_probs(slimm::lzip::kLc, slimm::lzip::kLp)) return 3;
    if (argc == 5 && strcmp(argv[1], "--damage") == 0) {
        if (!damage::slurp(argv[4], blob) || blob.empty()) return 2;
        int ok = 0, errors = 0;
        auto one = [&](const std::vector<uint8_t>& b) {
            uint64_t n = 0;
            uint32_t h = 0;
            std::string err;
            const bool good = decode(b, nullptr, n, h, err, nullptr);
            walk(b, 0, nullptr);
            walk(b, 1000, nullptr);
            index(b, nullptr);
            if (!good && err.empty()) {
                fprintf(stderr, "an error without words\n");
                exit(1);
            }
            ++(good ? ok : errors);
        };
        damage::device_trials(blob, strtoull(argv[2], nullptr, 10), atoi(argv[3]), [&](int, const std::vector<uint8_t>& b) { one(b); });
        for (size_t n = 0; n < std::min<size_t>(blob.size(), 300); ++n) one(std::vector<uint8_t>(blob.begin(), blob.begin() + static_cast<long>(n)));
        printf("ok=%d errors=%d total=%d\n", ok, errors, ok + errors);
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--walk") == 0) {
        if (!damage::slurp(argv[2], blob)) return 2;
        walk(blob, 0, stdout);
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "--feed") == 0) {
        if (!damage::slurp(argv[3], blob)) return 2;
        walk(blob, static_cast<size_t>(std::max(1, atoi(argv[2]))), stdout);
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--index") == 0) {
        if (!damage::slurp(argv[2], blob)) return 2;
        index(blob, stdout);
        return 0;
    }
    if (argc == 4 && (strcmp(argv[1], "--out") == 0 || strcmp(argv[1], "--members") == 0)) {
        if (!damage::slurp(argv[3], blob)) return 2;
        std::vector<uint8_t> text;
        uint64_t n = 0;
        uint32_t h = 0;
        std::string err;
        if (!decode(blob, &text, n, h, err, nullptr)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        if (strcmp(argv[1], "--out") == 0) {
            FILE* f = fopen(argv[2], "wb");
            if (!f || fwrite(text.data(), 1, text.size(), f) != text.size()) return 2;
            fclose(f);
            return 0;
        }
        // (the members' extents by the walker, their texts cut from the whole by the stated sizes)
        Walker w;
        uint64_t pos = 0, at = 0;
        for (int k = 0;; ++k) {
            const Walker::Item it = w.peek(blob.data() + pos, blob.size() - pos, pos, true);
            if (it.kind != Walker::MemberItem) break;
            FILE* f = fopen((std::string(argv[2]) + "." + std::to_string(k)).c_str(), "wb");
            if (!f || fwrite(text.data() + at, 1, it.trailer.data_size, f) != it.trailer.data_size) return 2;
            fclose(f);
            at += it.trailer.data_size;
            w.take(it);
            pos += it.bytes;
        }
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        uint64_t n = 0;
        uint32_t h = 0;
        std::string err;
        slimm::LzipReader::Counts c;
        blob.clear();
        if (!damage::slurp(argv[i], blob)) err = "cannot open";
        if (err.empty() && decode(blob, nullptr, n, h, err, &c))
            printf("%s\tok\t%llu\t%08x\t%llu %llu %llu %llu %llu\n", argv[i], (unsigned long long)n, h, (unsigned long long)c.members,
                   (unsigned long long)c.empty_members, (unsigned long long)c.match_bytes, (unsigned long long)c.max_dist, (unsigned long long)c.max_dict);
        else
            printf("%s\terror\t%s\n", argv[i], err.c_str());
    }
    return 0;
}
