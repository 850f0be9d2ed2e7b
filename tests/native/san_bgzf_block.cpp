// TEST INFRASTRUCTURE ONLY: slimm_amd/csrc/bgzf_block.h by itself, built under AddressSanitizer and UBSan by
// tests/test_bgzf_block.py and scripts/sanitize_host.sh.  Every block is handed to block_at in a heap buffer of exactly the
// bytes it is told about, so that one read too far is a sanitizer report.  Prints "<case>\tok" or "<case>\tFAILED ..." per
// case; exit status 1 when any case failed.
#include "../../slimm_amd/csrc/bgzf_block.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace slimm;
using Bytes = std::vector<uint8_t>;

static int g_failed = 0;

static void report(const std::string& name, bool ok, const std::string& why = "") {
    printf("%s\t%s%s\n", name.c_str(), ok ? "ok" : "FAILED ", ok ? "" : why.c_str());
    g_failed += ok ? 0 : 1;
}

static const char* word(bgzf::Status s) {
    switch (s) {
        case bgzf::kOk: return "ok";
        case bgzf::kMore: return "more";
        case bgzf::kNotBgzf: return "not-bgzf";
        case bgzf::kNoBc: return "no-bc";
        case bgzf::kBadSize: return "bad-size";
        case bgzf::kTooLarge: return "too-large";
    }
    return "?";
}

static void put16(Bytes& b, uint32_t v) {
    b.push_back(static_cast<uint8_t>(v));
    b.push_back(static_cast<uint8_t>(v >> 8));
}
static void put32(Bytes& b, uint32_t v) {
    put16(b, v & 0xffffu);
    put16(b, v >> 16);
}
static Bytes subfield(char a, char b, const Bytes& data) {
    Bytes f = {static_cast<uint8_t>(a), static_cast<uint8_t>(b)};
    put16(f, static_cast<uint32_t>(data.size()));
    f.insert(f.end(), data.begin(), data.end());
    return f;
}
static const Bytes kBcSlot = {'B', 'C', 2, 0, 0, 0};   // BC with room for BSIZE

// A block with the extra field `extra` (its first BC subfield's BSIZE set to `bsize`, or to the block's own when bsize < 0),
// `payload` as its deflate data, and the trailer
static Bytes block(const Bytes& extra, const Bytes& payload, uint32_t crc, uint32_t isize, long bsize = -1) {
    Bytes b = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
    put16(b, static_cast<uint32_t>(extra.size()));
    b.insert(b.end(), extra.begin(), extra.end());
    b.insert(b.end(), payload.begin(), payload.end());
    put32(b, crc);
    put32(b, isize);
    const uint32_t v = bsize < 0 ? static_cast<uint32_t>(b.size() - 1) : static_cast<uint32_t>(bsize);
    for (size_t o = 12; o + 6 <= 12 + extra.size(); ++o)
        if (memcmp(&b[o], kBcSlot.data(), 4) == 0) {
            b[o + 4] = static_cast<uint8_t>(v);
            b[o + 5] = static_cast<uint8_t>(v >> 8);
            break;
        }
    return b;
}

// block_at over the first `avail` bytes of `b`, copied into a heap buffer of exactly that size
static bgzf::Status at(const Bytes& b, size_t avail, bgzf::Header* h) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[avail]);
    if (avail) memcpy(p.get(), b.data(), avail);
    return bgzf::block_at(p.get(), avail, h);
}

static void expect(const std::string& name, const Bytes& b, bgzf::Status want) {
    bgzf::Header h{};
    const bgzf::Status got = at(b, b.size(), &h);
    report(name, got == want, std::string("got ") + word(got) + ", want " + word(want));
}

// kOk with the five fields at the block's full size, kMore at every size below it
static void expect_whole(const std::string& name, const Bytes& b, uint32_t xlen, uint32_t csize, uint32_t crc, uint32_t isize, bool every_prefix) {
    bgzf::Header h{};
    const bgzf::Status got = at(b, b.size(), &h);
    const bool fields = h.xlen == xlen && h.total == b.size() && h.csize == csize && h.crc == crc && h.isize == isize;
    report(name, got == bgzf::kOk && fields, std::string("got ") + word(got) + (fields ? "" : ", wrong fields"));
    if (!every_prefix) return;
    size_t wrong = 0;
    for (size_t avail = 0; avail < b.size(); ++avail) wrong += at(b, avail, &h) != bgzf::kMore;
    report(name + "/every-prefix", wrong == 0, std::to_string(wrong) + " prefixes did not answer more");
}

static void eof_block(const std::string& name, const Bytes& b, bool want) {
    bgzf::Header h{};
    const bgzf::Status st = at(b, b.size(), &h);
    std::unique_ptr<uint8_t[]> payload(new uint8_t[h.csize ? h.csize : 1]);
    if (st == bgzf::kOk) memcpy(payload.get(), b.data() + 12 + h.xlen, h.csize);
    const bool got = st == bgzf::kOk && bgzf::is_eof_block(payload.get(), h.csize, h.isize, h.crc);
    report(name, st == bgzf::kOk && got == want, std::string("status ") + word(st) + ", is_eof_block " + (got ? "true" : "false"));
}

int main() {
    Bytes data(300);
    for (size_t i = 0; i < data.size(); ++i) data[i] = static_cast<uint8_t>(i * 7 + 3);
    const Bytes front = subfield('X', 'Y', {1, 2, 3}), behind = subfield('Z', 'Z', {9, 8, 7, 6, 5});
    auto cat = [](std::initializer_list<Bytes> parts) {
        Bytes all;
        for (const Bytes& p : parts) all.insert(all.end(), p.begin(), p.end());
        return all;
    };
    const uint32_t crc = 0x89abcdefu;

    expect_whole("canonical", block(kBcSlot, data, crc, 1000), 6, 300, crc, 1000, true);
    expect_whole("subfield-in-front", block(cat({front, kBcSlot}), data, crc, 1000), 13, 300, crc, 1000, false);
    expect_whole("subfield-behind", block(cat({kBcSlot, behind}), data, crc, 1000), 15, 300, crc, 1000, false);
    expect_whole("subfields-on-both-sides", block(cat({front, kBcSlot, behind}), data, crc, 1000), 22, 300, crc, 1000, true);
    // (BC as the last subfield: o + 6 == xlen, its last byte the extra field's last)
    expect_whole("bc-last", block(cat({front, front, kBcSlot}), data, crc, 1000), 20, 300, crc, 1000, false);
    expect_whole("empty-payload", block(kBcSlot, {}, 0, 0), 6, 0, 0, 0, false);

    expect("bc-of-three-bytes", block(subfield('B', 'C', {1, 2, 3}), data, crc, 1000), bgzf::kNoBc);
    expect("bc-of-no-bytes", block(subfield('B', 'C', {}), data, crc, 1000), bgzf::kNoBc);
    expect("other-subfields-only", block(cat({front, behind}), data, crc, 1000), bgzf::kNoBc);
    expect("xlen-0", block({}, data, crc, 1000), bgzf::kNoBc);
    {   // a subfield whose SLEN runs past XLEN, in front of where BC would lie and as the extra field's only one
        Bytes long_one = front;
        long_one[2] = 200;
        expect("slen-past-xlen", block(cat({long_one, kBcSlot}), data, crc, 1000), bgzf::kNoBc);
        expect("slen-past-xlen-alone", block(long_one, data, crc, 1000), bgzf::kNoBc);
        Bytes cut = {'B', 'C', 2, 0, 0};   // a BC whose second BSIZE byte lies behind the extra field
        expect("bc-cut-by-xlen", block(cut, data, crc, 1000), bgzf::kNoBc);
    }
    expect("bsize-below-header-and-trailer", block(kBcSlot, data, crc, 1000, 12 + 6 + 8 - 2), bgzf::kBadSize);
    expect("bsize-0", block(kBcSlot, data, crc, 1000, 0), bgzf::kBadSize);
    expect_whole("bsize-of-header-and-trailer", block(kBcSlot, {}, crc, 5), 6, 0, crc, 5, false);
    expect("bsize-beyond-the-bytes", block(kBcSlot, data, crc, 1000, 12 + 6 + 300 + 8), bgzf::kMore);
    expect_whole("isize-65536", block(kBcSlot, data, crc, 65536), 6, 300, crc, 65536, false);
    expect("isize-65537", block(kBcSlot, data, crc, 65537), bgzf::kTooLarge);
    expect("isize-2^32-1", block(kBcSlot, data, crc, 0xffffffffu), bgzf::kTooLarge);
    for (int k = 0; k < 4; ++k) {
        Bytes b = block(kBcSlot, data, crc, 1000);
        b[k] = k == 3 ? 0xfb : static_cast<uint8_t>(b[k] + 1);   // (FLG: every bit but FEXTRA)
        expect("wrong-byte-" + std::to_string(k), b, bgzf::kNotBgzf);
        b.resize(12);   // ... which shows with the fixed part of the header alone
        expect("wrong-byte-" + std::to_string(k) + "/12-bytes", b, bgzf::kNotBgzf);
    }
    {   // FLG with other bits beside FEXTRA is still a block
        Bytes b = block(kBcSlot, data, crc, 1000);
        b[3] = 0x1c;
        expect("flg-with-more-bits", b, bgzf::kOk);
    }

    const Bytes eof = block(kBcSlot, {0x03, 0x00}, 0, 0);
    report("eof-block-is-28-bytes", eof.size() == 28);
    eof_block("eof-block", eof, true);
    eof_block("eof-block-behind-subfields", block(cat({front, kBcSlot, behind}), {0x03, 0x00}, 0, 0), true);
    eof_block("eof-near-miss-crc", block(kBcSlot, {0x03, 0x00}, 1, 0), false);
    eof_block("eof-near-miss-payload", block(kBcSlot, {0x03, 0x01}, 0, 0), false);
    eof_block("eof-near-miss-isize", block(kBcSlot, {0x03, 0x00}, 0, 1), false);
    eof_block("eof-near-miss-three-bytes", block(kBcSlot, {0x03, 0x00, 0x00}, 0, 0), false);

    printf("failed\t%d\n", g_failed);
    return g_failed ? 1 : 0;
}
