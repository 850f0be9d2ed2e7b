// The host lz4 decoder and the container walker (slimm_amd/csrc/host/lz4.cpp, lz4_frame.h, lz4_walk.h) as a stand-alone
// program, for the sanitizer pass and the CPU tests (tests/test_lz4_frame.py, tests/test_lz4_sanitized.py):
//   san_lz4 FILE...              every file decoded: "FILE<tab>ok<tab>bytes<tab>xxh32" or "FILE<tab>error<tab>message"
//   san_lz4 --out OUT FILE       the decoded bytes of FILE into OUT (exit 1 + the message on an error)
//   san_lz4 --xxh32 PIECE FILE   XXH32 of FILE's bytes, taken PIECE bytes at a time
//   san_lz4 --walk FILE          the container's items by lz4::Walker over the whole file, one a line:
//                                "skippable AT", "frame AT linked block_sums content_size|- block_max", "block AT stored size",
//                                "end AT", "sum AT", and "error <words>" where it stops
//   san_lz4 --block MAX FILE     FILE as one compressed block: "ok<tab>bytes<tab>hex of the text" or "error<tab>words"
//   san_lz4 --damage SEED N FILE N damaged copies of FILE (a bit flipped, the file cut short, a stretch copied elsewhere:
//                                damaged_copies.h) and every truncation of its first 300 bytes, decoded and walked:
//                                "ok=a errors=b total=c"
// Damaged input must end in an error message, never in a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../slimm_amd/csrc/host/lz4.hpp"
#include "damaged_copies.h"

using slimm::lz4::Walker;

static bool decode(const std::vector<uint8_t>& b, std::vector<uint8_t>* keep, uint64_t& n, uint32_t& hash, std::string& err) {
    size_t fed = 0;
    slimm::Lz4Reader r([&](uint8_t* d, size_t cap) {
        const size_t k = std::min(cap, b.size() - fed);
        if (k) memcpy(d, b.data() + fed, k);
        fed += k;
        return k;
    });
    slimm::lz4::Xxh32 x;
    std::vector<uint8_t> buf(77777);   // (no multiple of a block's size: reads end inside blocks)
    long got;
    n = 0;
    while ((got = r.read(buf.data(), buf.size())) > 0) {
        x.update(buf.data(), static_cast<uint64_t>(got));
        if (keep) keep->insert(keep->end(), buf.begin(), buf.begin() + got);
        n += static_cast<uint64_t>(got);
    }
    hash = x.digest();
    if (got < 0) err = r.error();
    return got == 0;
}

// the walker over the whole of b; `out`: where the lines go (null: nowhere)
static bool walk(const std::vector<uint8_t>& b, FILE* out) {
    Walker w;
    uint64_t pos = 0;
    for (;;) {
        const Walker::Item it = w.peek(b.data() + pos, b.size() - pos, pos);
        if (it.kind == Walker::MayEnd) return true;
        if (it.kind == Walker::More || it.kind == Walker::Error) {
            if (out) fprintf(out, "error %s\n", it.words().c_str());
            return false;
        }
        if (out) {
            const unsigned long long at = it.at;
            if (it.kind == Walker::SkippableFrame) fprintf(out, "skippable %llu\n", at);
            if (it.kind == Walker::Header) {
                fprintf(out, "frame %llu %d %d ", at, it.fh.linked, it.fh.block_sums);
                if (it.fh.has_size) fprintf(out, "%llu", (unsigned long long)it.fh.content_size);
                else fprintf(out, "-");
                fprintf(out, " %u\n", it.fh.block_max);
            }
            if (it.kind == Walker::Block) fprintf(out, "block %llu %d %u\n", at, it.stored, it.size);
            if (it.kind == Walker::EndMark) fprintf(out, "end %llu\n", at);
            if (it.kind == Walker::Sum) fprintf(out, "sum %llu\n", at);
        }
        w.take(it);
        pos += it.bytes;
    }
}

int main(int argc, char** argv) {
    std::vector<uint8_t> blob;
    if (argc == 5 && strcmp(argv[1], "--damage") == 0) {
        if (!damage::slurp(argv[4], blob) || blob.empty()) return 2;
        int ok = 0, errors = 0;
        auto one = [&](const std::vector<uint8_t>& b) {
            uint64_t n = 0;
            uint32_t h = 0;
            std::string err;
            const bool good = decode(b, nullptr, n, h, err);
            walk(b, nullptr);
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
    if (argc == 4 && strcmp(argv[1], "--xxh32") == 0) {
        if (!damage::slurp(argv[3], blob)) return 2;
        const size_t piece = static_cast<size_t>(std::max(1, atoi(argv[2])));
        slimm::lz4::Xxh32 x;
        for (size_t at = 0; at < blob.size(); at += piece) x.update(blob.data() + at, std::min(piece, blob.size() - at));
        printf("%08x\n", x.digest());
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--walk") == 0) {
        if (!damage::slurp(argv[2], blob)) return 2;
        walk(blob, stdout);
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "--block") == 0) {
        if (!damage::slurp(argv[3], blob)) return 2;
        std::vector<uint8_t> text;
        const uint32_t st = slimm::Lz4Reader::decode_block(blob.data(), static_cast<uint32_t>(blob.size()), static_cast<uint32_t>(atoi(argv[2])), text, 0);
        if (st != slimm::lz4::kOk) {
            printf("error\t%s\n", slimm::lz4::status_text(st));
            return 0;
        }
        printf("ok\t%zu\t", text.size());
        for (uint8_t c : text) printf("%02x", c);
        printf("\n");
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "--out") == 0) {
        if (!damage::slurp(argv[3], blob)) return 2;
        std::vector<uint8_t> text;
        uint64_t n = 0;
        uint32_t h = 0;
        std::string err;
        if (!decode(blob, &text, n, h, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        FILE* f = fopen(argv[2], "wb");
        if (!f || fwrite(text.data(), 1, text.size(), f) != text.size()) return 2;
        fclose(f);
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        uint64_t n = 0;
        uint32_t h = 0;
        std::string err;
        if (!damage::slurp(argv[i], blob)) err = "cannot open";
        if (err.empty() && decode(blob, nullptr, n, h, err)) printf("%s\tok\t%llu\t%08x\n", argv[i], (unsigned long long)n, h);
        else printf("%s\terror\t%s\n", argv[i], err.c_str());
    }
    return 0;
}
