// The record filter's host functions (slimm_host_record_passes_bam / _sam: slimm_amd/csrc/record_filter.h, the lines the
// library itself compiles) as a stand-alone program for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wextra tests/native/san_record_filter.cpp -o san_record_filter
//   san_record_filter [SEED]
// BAM records and SAM lines it writes itself -- CIGARs of up to 40 operations, tag areas with every value type, NM of every
// integer type in front of, between and behind them -- are judged whole, and then damaged at random: lengths overstated
// (l_read_name, n_cigar_op, l_seq, a B array's count), tag types unknown, strings without their NUL, records and lines cut
// short, bytes overwritten.  Every record is judged in a heap allocation of exactly its size, so a read outside it is
// reported.  Every answer must be 1 (kept) or 0 (dropped) with a `why` that fits it.  Prints one line; exit status 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define SLIMM_RF_HOST_API
#include "../../slimm_amd/csrc/record_filter.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return static_cast<uint32_t>((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0u; }

static void put16(std::vector<uint8_t>& b, uint32_t v) { b.push_back(v & 255u), b.push_back((v >> 8) & 255u); }
static void put32(std::vector<uint8_t>& b, uint32_t v) { put16(b, v & 0xffffu), put16(b, v >> 16); }
static void set32(std::vector<uint8_t>& b, size_t at, uint32_t v) {
    for (int k = 0; k < 4; ++k) b[at + k] = (v >> (8 * k)) & 255u;
}

struct Made {
    std::vector<uint8_t> bam;   // the record behind its block_size word
    std::string sam;            // the line, without a newline
    size_t tags_at = 0;         // where the BAM record's tag area starts
};

static Made make_record() {
    Made m;
    const uint32_t flag = (rnd() & 0xffbu) | (below(8) ? 0u : 4u), mapq = below(4) ? below(61) : 255u, l_seq = below(160);
    const std::string name = "read/" + std::to_string(rnd() % 100000u);
    const char* ops = "MIDNSHP=X";
    std::vector<std::pair<uint32_t, uint32_t>> cigar;
    for (uint32_t k = below(5) ? below(41) : 0u; k; --k) cigar.emplace_back(1u + below(60), below(9));
    std::vector<uint8_t>& b = m.bam;
    put32(b, below(8)), put32(b, below(100000));
    b.push_back(static_cast<uint8_t>(name.size() + 1)), b.push_back(static_cast<uint8_t>(mapq));
    put16(b, 4680), put16(b, static_cast<uint32_t>(cigar.size())), put16(b, flag), put32(b, l_seq);
    put32(b, 0xffffffffu), put32(b, 0xffffffffu), put32(b, 0);
    b.insert(b.end(), name.begin(), name.end()), b.push_back(0);
    std::string ctext;
    for (auto& c : cigar) put32(b, (c.first << 4) | c.second), ctext += std::to_string(c.first) + ops[c.second];
    for (uint32_t k = 0; k < (l_seq + 1) / 2 + l_seq; ++k) b.push_back(static_cast<uint8_t>(rnd()));
    m.tags_at = b.size();
    m.sam = name + "\t" + std::to_string(flag) + "\tref" + std::to_string(below(8)) + "\t" + std::to_string(1 + below(100000)) + "\t" +
            std::to_string(mapq) + "\t" + (ctext.empty() ? "*" : ctext) + "\t*\t0\t0\t" + (l_seq ? std::string(l_seq, 'A') : "*") + "\t*";
    const uint32_t n_tags = below(7), nm_at = below(3) ? below(n_tags + 1) : 99u;
    for (uint32_t k = 0; k <= n_tags; ++k) {
        if (k == nm_at) {
            const char ty = "cCsSiI"[below(6)];
            const uint32_t v = below(ty == 'c' ? 128u : 200u);
            b.push_back('N'), b.push_back('M'), b.push_back(static_cast<uint8_t>(ty));
            if (ty == 'c' || ty == 'C') b.push_back(static_cast<uint8_t>(v));
            else if (ty == 's' || ty == 'S') put16(b, v);
            else put32(b, v);
            m.sam += "\tNM:i:" + std::to_string(v);
        }
        if (k == n_tags) break;
        b.push_back('X'), b.push_back(static_cast<uint8_t>('A' + k));
        switch (below(6)) {
        case 0: b.push_back('A'), b.push_back('U'), m.sam += "\tX" + std::string(1, 'A' + k) + ":A:U"; break;
        case 1: b.push_back('f'), put32(b, 0x3f000000u), m.sam += "\tX" + std::string(1, 'A' + k) + ":f:0.5"; break;
        case 2: b.push_back('i'), put32(b, rnd()), m.sam += "\tX" + std::string(1, 'A' + k) + ":i:7"; break;
        case 3: case 4: {
            const bool hex = below(2) != 0;
            std::string v;
            for (uint32_t j = below(200) & ~1u; j; --j) v += "0123456789ABCDEF"[below(16)];
            b.push_back(hex ? 'H' : 'Z'), b.insert(b.end(), v.begin(), v.end()), b.push_back(0);
            m.sam += "\tX" + std::string(1, 'A' + k) + (hex ? ":H:" : ":Z:") + v;
            break;
        }
        default: {
            const char sub = "cCsSiIf"[below(7)];
            const uint32_t cnt = below(40), es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : 4u;
            b.push_back('B'), b.push_back(static_cast<uint8_t>(sub)), put32(b, cnt);
            for (uint32_t j = 0; j < cnt * es; ++j) b.push_back(static_cast<uint8_t>(rnd()));
            m.sam += "\tX" + std::string(1, 'A' + k) + ":B:" + sub;
            for (uint32_t j = 0; j < cnt; ++j) m.sam += ",1";
        }
        }
    }
    return m;
}

static unsigned long long g_answers[7] = {};

static void check(int rc, int why) {
    if ((rc != 0 && rc != 1) || why < 0 || why > 6 || (rc == 0) != (why >= 1 && why <= 5)) {
        fprintf(stderr, "san_record_filter: answer %d with why %d\n", rc, why);
        abort();
    }
    ++g_answers[why];
}

// in an allocation of exactly n bytes, against every filter
static void judge(const std::vector<slimm_record_filter>& filters, const uint8_t* bytes, size_t n, bool bam) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) memcpy(exact.get(), bytes, n);
    for (const slimm_record_filter& f : filters) {
        int why = -1;
        const int rc = bam ? slimm_host_record_passes_bam(&f, exact.get(), static_cast<uint32_t>(n), &why)
                           : slimm_host_record_passes_sam(&f, reinterpret_cast<const char*>(exact.get()), static_cast<uint32_t>(n), &why);
        check(rc, why);
    }
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 10) * 0xff51afd7ed558ccdull + 1u;
    std::vector<slimm_record_filter> filters(6);
    memset(filters.data(), 0, filters.size() * sizeof(slimm_record_filter));
    filters[1].min_mapq = 10;
    filters[2].require_flags = 0x2, filters[2].exclude_flags = 0xf00;
    filters[3].min_aligned = 50;
    filters[4].min_identity_permille = 950;
    filters[5].min_mapq = 1, filters[5].exclude_flags = 0x400, filters[5].min_aligned = 1, filters[5].min_identity_permille = 1000;
    {   // what the setters refuse, the host functions refuse too
        slimm_record_filter bad = filters[1];
        bad.min_identity_permille = 1001;
        const uint8_t z[36] = {};
        if (slimm_host_record_passes_bam(&bad, z, 36, nullptr) != -1 || slimm_host_record_passes_sam(nullptr, "x", 1, nullptr) != -1) abort();
    }
    unsigned long long whole = 0, damaged = 0;
    for (int round = 0; round < 3000; ++round) {
        const Made m = make_record();
        judge(filters, m.bam.data(), m.bam.size(), true);
        judge(filters, reinterpret_cast<const uint8_t*>(m.sam.data()), m.sam.size(), false);
        whole += 2;
        for (int d = 0; d < 12; ++d) {
            std::vector<uint8_t> b = m.bam;
            switch (below(8)) {
            case 0: b[8] = static_cast<uint8_t>(rnd()); break;                              // l_read_name
            case 1: b[12] = static_cast<uint8_t>(rnd()), b[13] = static_cast<uint8_t>(rnd()); break;   // n_cigar_op
            case 2: set32(b, 16, below(2) ? rnd() : 0xffffffffu); break;                    // l_seq
            case 3: b.resize(below(static_cast<uint32_t>(b.size()) + 1u)); break;           // cut short, down to nothing
            case 4:                                                                         // a tag type nobody knows
                if (m.tags_at + 3 <= b.size()) b[m.tags_at + 2] = static_cast<uint8_t>(rnd());
                break;
            case 5:                                                                         // a B count (or whatever lies there): huge
                for (size_t p = m.tags_at; p + 8 <= b.size(); ++p)
                    if (b[p] == 'B' && below(2)) set32(b, p + 2, 0xfffffff0u | below(16));
                break;
            case 6:                                                                         // strings lose their NULs
                for (size_t p = m.tags_at; p < b.size(); ++p)
                    if (b[p] == 0) b[p] = 'x';
                break;
            default:
                for (uint32_t k = 1 + below(6); k && !b.empty(); --k) b[below(static_cast<uint32_t>(b.size()))] = static_cast<uint8_t>(rnd());
            }
            judge(filters, b.data(), b.size(), true);
            std::string s = m.sam;
            switch (below(5)) {
            case 0: s.resize(below(static_cast<uint32_t>(s.size()) + 1u)); break;
            case 1: for (char& c : s) if (c == '\t' && !below(4)) c = ' '; break;
            case 2: if (!s.empty()) s[below(static_cast<uint32_t>(s.size()))] = '\n'; break;
            case 3: s += "\tNM:i:"; s += below(2) ? "-" : "99999999999999999999999999"; break;
            default:
                for (uint32_t k = 1 + below(6); k && !s.empty(); --k) s[below(static_cast<uint32_t>(s.size()))] = static_cast<char>(rnd());
            }
            judge(filters, reinterpret_cast<const uint8_t*>(s.data()), s.size(), false);
            damaged += 2;
        }
    }
    for (int k = 0; k < 7; ++k)
        if (!g_answers[k]) {
            fprintf(stderr, "san_record_filter: no answer with why %d\n", k);
            return 1;
        }
    printf("%llu whole and %llu damaged records judged: ok\n", whole, damaged);
    return 0;
}
