// `slimm [OPTIONS] DB.sldb IN` -- the reference's command line (reference src/slimm.cpp:60-204) on top of the C ABI.
//
// Same options, defaults and output files as the reference; the per-file driver follows slimm::get_profiles()
// (reference src/slimm.hpp:395-496) step for step, with the three hot phases running on the MI355X through
// include/slimm_hip.h.  Extra options (no reference counterpart): --device N, --query-grouped, --any-order,
// --dump-records (decode only, for reader tests on machines without a GPU), --devices with --split-input (one file over
// several devices) or with --file-per-device (the files of a directory side by side, one per listed device).
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/mman.h>
#include <ctime>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <mutex>
#include <numeric>
#include <shared_mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/slimm_hip.h"
#include <dlfcn.h>

// ---------------------------------------------------------------------------------------------------------------
// libslimm_hip.so behind its own names, loaded late.  Linking the library the ordinary way makes the dynamic loader map
// it -- and the HIP runtime under it -- before main() starts: 0.12 s in which nothing else happens.  Here a thread of its
// own dlopen()s the library (and starts the HIP runtime, slimm_warm_up) while main() parses its options, loads the
// database, samples the read length and starts decoding; the forwarders below wait for that thread the first time the
// library is needed.  Call sites stay what they would be with the library linked in (INTEGRATION.md shows that form).
// ---------------------------------------------------------------------------------------------------------------
namespace lazy {
std::mutex mu;
std::condition_variable cv;
void* handle = nullptr;
bool done = false;
std::string error;

std::string library_path() {
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
    std::string dir = n > 0 ? std::string(exe, static_cast<size_t>(n)) : std::string("./slimm");
    dir = dir.substr(0, dir.find_last_of('/') + 1);
    if (const char* e = getenv("SLIMM_HIP_LIB")) return e;
    return dir + "libslimm_hip.so";
}
void load(const std::vector<int>& devices) {  // (the devices of --devices start side by side: a thread each)
    void* h = dlopen(library_path().c_str(), RTLD_NOW | RTLD_LOCAL);
    std::string err = h ? "" : dlerror();
    if (h) {
        auto warm = reinterpret_cast<int (*)(int)>(dlsym(h, "slimm_warm_up"));
        std::vector<std::thread> others;
        for (size_t i = 1; warm && i < devices.size(); ++i)
            if (std::find(devices.begin(), devices.begin() + static_cast<long>(i), devices[i]) == devices.begin() + static_cast<long>(i))
                others.emplace_back([warm, d = devices[i]] { (void)warm(d); });
        if (warm && !devices.empty()) (void)warm(devices[0]);
        for (auto& t : others) t.join();
    }
    std::lock_guard<std::mutex> g(mu);
    handle = h;
    error = err;
    done = true;
    cv.notify_all();
}
void* symbol(const char* name) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [] { return done; });
    void* f = handle ? dlsym(handle, name) : nullptr;
    if (!f) {
        std::cerr << "slimm: cannot use " << library_path() << " (" << (handle ? name : error.c_str()) << ")\n";
        _exit(1);
    }
    return f;
}
}  // namespace lazy

#define SLIMM_FORWARD(ret, name, params, args)                                       \
    extern "C" ret name params {                                                     \
        static const auto f = reinterpret_cast<ret(*) params>(lazy::symbol(#name)); \
        return f args;                                                               \
    }
SLIMM_FORWARD(int, slimm_create, (const slimm_config* a, slimm_ctx** b), (a, b))
SLIMM_FORWARD(int, slimm_set_input_size_hint, (slimm_ctx* a, uint64_t b), (a, b))
SLIMM_FORWARD(int, slimm_device_memory, (slimm_ctx* a, uint64_t* b, uint64_t* c), (a, b, c))
SLIMM_FORWARD(int, slimm_window_memory, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(void, slimm_destroy, (slimm_ctx* a), (a))
SLIMM_FORWARD(const char*, slimm_last_error, (const slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_get_cutoff_cache, (slimm_ctx* a, float* b, float* c), (a, b, c))
SLIMM_FORWARD(int, slimm_set_cutoff_cache, (slimm_ctx* a, float b, float c), (a, b, c))
SLIMM_FORWARD(int, slimm_push_records,
              (slimm_ctx* a, const uint64_t* b, const int32_t* c, const int32_t* d, const uint16_t* e, uint64_t f_), (a, b, c, d, e, f_))
SLIMM_FORWARD(int, slimm_push_records_checked,
              (slimm_ctx* a, const uint64_t* b, const int32_t* c, const int32_t* d, const uint16_t* e, const uint32_t* f_, uint64_t g),
              (a, b, c, d, e, f_, g))
SLIMM_FORWARD(int, slimm_staging_buffers,
              (slimm_ctx* a, uint32_t b, uint64_t c, uint64_t** d, int32_t** e, int32_t** f_, uint16_t** g), (a, b, c, d, e, f_, g))
SLIMM_FORWARD(int, slimm_push_staged_async, (slimm_ctx* a, uint32_t b, uint64_t c), (a, b, c))
SLIMM_FORWARD(int, slimm_push_staged_packed_async, (slimm_ctx* a, uint32_t b, uint64_t c), (a, b, c))
SLIMM_FORWARD(int, slimm_push_staged_marked_async, (slimm_ctx* a, uint32_t b, uint64_t c), (a, b, c))
SLIMM_FORWARD(int, slimm_push_records_marked, (slimm_ctx* a, const uint32_t* b, const int32_t* c, uint64_t d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_group_push_records_marked, (slimm_group* a, const uint32_t* b, const int32_t* c, uint64_t d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_set_reference_names, (slimm_ctx * c, const char* const* names), (c, names))
SLIMM_FORWARD(int, slimm_push_sam_bytes, (slimm_ctx * c, const uint8_t* t, uint64_t n, int last, uint64_t* got), (c, t, n, last, got))
SLIMM_FORWARD(void, slimm_mark_words,
              (const uint64_t* a, const uint16_t* b, const int32_t* c, uint64_t d, const uint64_t* e, uint32_t* f_), (a, b, c, d, e, f_))
SLIMM_FORWARD(int, slimm_push_records_packed, (slimm_ctx* a, const uint64_t* b, const int32_t* c, const int32_t* d, uint64_t e),
              (a, b, c, d, e))
SLIMM_FORWARD(int, slimm_push_bam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, int d, uint64_t* e), (a, b, c, d, e))
SLIMM_FORWARD(int, slimm_push_bgzf_blocks, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_push_bgzf_sam_blocks, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_push_bzip2_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_push_gzip_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_get_gzip_stats, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_push_zstd_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_get_zstd_stats, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_push_lz4_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_get_lz4_stats, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_push_lzip_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_get_lzip_stats, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_host_lzip_members, (const char* a, uint64_t* b, uint64_t* c), (a, b, c))
SLIMM_FORWARD(int, slimm_push_xz_sam_bytes, (slimm_ctx* a, const uint8_t* b, uint64_t c, uint32_t s, int d, uint64_t* e), (a, b, c, s, d, e))
SLIMM_FORWARD(int, slimm_get_xz_stats, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_pin_host_buffer, (slimm_ctx* a, const void* b, uint64_t c), (a, b, c))
SLIMM_FORWARD(int, slimm_host_bgzf_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_host_text_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_set_input_mid_file, (slimm_ctx* a, int b, int c), (a, b, c))
SLIMM_FORWARD(int, slimm_host_bzip2_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_set_input_range, (slimm_ctx* a, uint64_t b, uint64_t c), (a, b, c))
SLIMM_FORWARD(uint64_t, slimm_bzip2_split_slack, (), ())
SLIMM_FORWARD(int, slimm_host_zstd_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(uint64_t, slimm_zstd_split_floor, (), ())
SLIMM_FORWARD(int, slimm_host_xz_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_host_xz_check_at, (const char* a, uint64_t b, int* c), (a, b, c))
SLIMM_FORWARD(int, slimm_set_xz_range_check, (slimm_ctx* a, int b), (a, b))
SLIMM_FORWARD(uint64_t, slimm_xz_split_floor, (), ())
SLIMM_FORWARD(int, slimm_host_gzip_ranges, (const char* a, uint64_t b, uint32_t c, uint64_t* d), (a, b, c, d))
SLIMM_FORWARD(int, slimm_set_gzip_range, (slimm_ctx* a, uint64_t b, uint64_t c), (a, b, c))
SLIMM_FORWARD(int, slimm_set_gzip_window_pass, (slimm_ctx* a, int b), (a, b))
SLIMM_FORWARD(int, slimm_group_gzip_windows, (slimm_group* a), (a))
SLIMM_FORWARD(uint64_t, slimm_gzip_split_floor, (), ())
SLIMM_FORWARD(int, slimm_group_stitch_ranges, (slimm_group* a), (a))
SLIMM_FORWARD(uint64_t, slimm_record_cap, (), ())
SLIMM_FORWARD(int, slimm_shutdown, (), ())
SLIMM_FORWARD(int, slimm_reset, (slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_check_grouping, (slimm_ctx* a, uint64_t* b), (a, b))
SLIMM_FORWARD(int, slimm_keep_bins, (slimm_ctx* a, int b), (a, b))
SLIMM_FORWARD(int, slimm_analyze_alignments, (slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_finish_coverage, (slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_filter_alignments, (slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_get_reads_lca_count, (slimm_ctx* a), (a))
SLIMM_FORWARD(int, slimm_get_propagation_order, (slimm_ctx* a, int* b, uint32_t* c, uint32_t d, uint32_t* e), (a, b, c, d, e))
SLIMM_FORWARD(int, slimm_set_propagation_walk, (slimm_ctx* a, int b), (a, b))
SLIMM_FORWARD(int, slimm_write_abundance_file, (slimm_ctx* a, const char* b), (a, b))
SLIMM_FORWARD(int, slimm_get_stats, (slimm_ctx* a, slimm_stats* b), (a, b))
SLIMM_FORWARD(int, slimm_get_ref_columns, (slimm_ctx* a, slimm_ref_columns* b), (a, b))
SLIMM_FORWARD(int, slimm_get_bins, (slimm_ctx* a, int b, uint32_t* c), (a, b, c))
SLIMM_FORWARD(int, slimm_group_create, (const slimm_config* a, const int* b, uint32_t c, slimm_group** d), (a, b, c, d))
SLIMM_FORWARD(void, slimm_group_destroy, (slimm_group* a), (a))
SLIMM_FORWARD(const char*, slimm_group_last_error, (const slimm_group* a), (a))
SLIMM_FORWARD(slimm_ctx*, slimm_group_context, (slimm_group* a, uint32_t b), (a, b))
SLIMM_FORWARD(int, slimm_group_uses_rccl, (const slimm_group* a), (a))
SLIMM_FORWARD(int, slimm_group_set_exchange, (slimm_group* a, int b), (a, b))
SLIMM_FORWARD(int, slimm_group_push_records_checked,
              (slimm_group* a, const uint64_t* b, const int32_t* c, const int32_t* d, const uint16_t* e, const uint32_t* f_, uint64_t g),
              (a, b, c, d, e, f_, g))
SLIMM_FORWARD(int, slimm_group_push_records_packed,
              (slimm_group * g, const uint64_t* k, const int32_t* r, const int32_t* p, uint64_t n), (g, k, r, p, n))
SLIMM_FORWARD(int, slimm_group_push_records,
              (slimm_group* a, const uint64_t* b, const int32_t* c, const int32_t* d, const uint16_t* e, uint64_t f_), (a, b, c, d, e, f_))
SLIMM_FORWARD(int, slimm_group_get_profiles, (slimm_group* a, const char* b), (a, b))
SLIMM_FORWARD(int, slimm_group_reset, (slimm_group* a), (a))
SLIMM_FORWARD(int, slimm_set_record_filter, (slimm_ctx* a, const slimm_record_filter* b), (a, b))
SLIMM_FORWARD(int, slimm_group_set_record_filter, (slimm_group* a, const slimm_record_filter* b), (a, b))
SLIMM_FORWARD(int, slimm_get_record_filter_stats, (slimm_ctx* a, uint64_t* b), (a, b))
#include "accession.hpp"
#include "alignment_file.hpp"
#include "zstd.hpp"
#include "xz.hpp"
#include "../force.h"
#include "../gzip_plan.h"
#include "../split_plan.h"
#include "sldb.hpp"

namespace {

using namespace slimm;

struct Options {  // arg_options, reference src/slimm.hpp:49-87
    float cov_cut_off = 0.95f, abundance_cut_off = 0.01f;
    uint32_t bin_width = 0, min_reads = 0;
    bool verbose = false, is_directory = false, raw_output = false, coverage_output = false;
    std::string rank = "species", input_path, output_prefix, database_path;
    // extensions
    int device = 0;
    std::vector<int> devices;  // --devices a,b,...: several GPUs, one process (slimm_group_*)
    int order = -1;  // -1: from the @HD line
    bool dump_records = false;
    bool dump_raw = false;   // --dump-raw: the inflated record bytes (AlignmentFile::read_raw), for reader tests without a GPU
    // how the records reach the device (defaults: the device inflates, finds and decodes; run-marked records for grouped files)
    bool host_decode = false;      // --host-decode: the host reader decodes the records (rounds 1 - 3's path)
    bool packed_records = false;   // --packed-records: 16-byte packed records instead of run-marked ones (host decoder)
    bool verify_grouping = false;  // --verify-grouping: count the read names that come back (slimm_check_grouping) and warn
    unsigned device_inflate = 1;   // --device-inflate K: every K-th window read in place is inflated on the device (0: none)
    unsigned window_mb = 0;        // --window-mb N: bytes per window buffer (tests make windows smaller than a record)
    int propagation_walk = SLIMM_WALK_DEFAULT;  // --propagation-walk default|reversed (include/slimm_hip.h, "THE ORDER OF THE PROPAGATION")
    bool split_input = false;      // --split-input (with --devices): every member reads its own byte range of the file, where its form is cut (kForms)
    // --file-per-device (with --devices): the listed devices are SLOTS that take whole files, one at a time, each through one
    // context on its device (run_file_per_device); parse() moves the list here and leaves `devices` empty: no group
    bool file_per_device = false;
    std::vector<int> slots;
    // -q, --require-flags, --exclude-flags, --min-aligned, --min-identity: one record filter for the whole run and every reader
    // (include/slimm_hip.h, "THE RECORD FILTER"); all zero: none
    slimm_record_filter filter{};
    bool filtered() const { return slimm_rf_on(&filter) != 0; }
};
bool g_trace = false;              // SLIMM_TRACE=cli (or all): millisecond marks of the stages on stderr

const char* kRankList[] = {"strains", "species", "genus", "family", "order", "class", "phylum", "superkingdom"};

// ---- reference src/file_helper.hpp:88-123 ----
std::string get_file_name(const std::string& s) { return s.substr(s.find_last_of("/\\") + 1); }
std::string get_directory(const std::string& s) { return s.substr(0, s.find_last_of("/\\")); }
std::string get_tsv_file_name(const std::string& prefix, const std::string& input) {
    std::string dir = get_directory(prefix), file = get_file_name(prefix);
    if (file.empty()) {
        file = get_file_name(input);
        auto ends = [&](const char* ext) {
            size_t p = file.find(ext);
            return p != std::string::npos && p == file.find_last_of(".");
        };
        if (ends(".sam") || ends(".bam")) file.replace(file.find_last_of("."), 4, "");
    }
    return dir + "/" + file;  // with no '/' in the prefix `dir` is the whole prefix (Q15)
}
std::string get_tsv_file_name(const std::string& prefix, const std::string& input, const std::string& suffix) {
    return get_tsv_file_name(prefix, input) + suffix + ".tsv";
}
std::vector<std::string> get_bam_files_in_directory(const std::string& directory) {  // src/file_helper.hpp:51-86
    std::vector<std::string> out;
    DIR* dir = opendir(directory.c_str());
    if (!dir) return out;
    while (dirent* ent = readdir(dir)) {
        const std::string name = ent->d_name, full = directory + "/" + name;
        if (name.empty() || name[0] == '.') continue;
        struct stat st;
        if (stat(full.c_str(), &st) == -1 || (st.st_mode & S_IFDIR)) continue;
        if (full.find(".sam") == full.find_last_of(".") || full.find(".bam") == full.find_last_of(".")) out.push_back(full);
    }
    closedir(dir);
    return out;
}

struct Lap {  // Timer<> of src/timer.hpp: whole seconds
    std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now(), lap_start = start;
    long lap() {
        auto now = std::chrono::steady_clock::now();
        long s = std::chrono::duration_cast<std::chrono::seconds>(now - lap_start).count();
        lap_start = now;
        return s;
    }
    long elapsed() const {
        return std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - start).count();
    }
};

void usage() {
    std::cerr << "slimm - Species Level Identification of Microbes from Metagenomes (MI355X path)\n"
                 "usage: slimm [OPTIONS] \"DB\" \"IN\"\n"
                 "  -o,  --output-prefix PREFIX   output path prefix (default: IN)\n"
                 "  -w,  --bin-width INT          width of a single bin in nucleotides (default 0 = average read length)\n"
                 "  -mr, --min-reads INT          minimum number of matching reads to consider a reference present\n"
                 "  -r,  --rank STRING            strains|species|genus|family|order|class|phylum|superkingdom (default species)\n"
                 "  -cc, --cov-cut-off DOUBLE     quantile of coverages used as cut-off, in [0, 1] (default 0.95)\n"
                 "  -ac, --abundance-cut-off DOUBLE  do not report abundances below this, in [0, 10] (default 0.01)\n"
                 "  -d,  --directory              IN is a directory of SAM/BAM files\n"
                 "  -ro, --raw-output             write raw reference statistics\n"
                 "  -co, --coverage-output        write raw coverage statistics\n"
                 "  -v,  --verbose\n"
                 "  -q,  --min-mapq INT           leave out alignments with MAPQ below INT, in [0, 255] (as samtools view -q)\n"
                 "       --require-flags INT      leave out alignments that lack one of these flag bits (samtools view -f; decimal or 0x...)\n"
                 "       --exclude-flags INT      leave out alignments with one of these flag bits (samtools view -F; decimal or 0x...)\n"
                 "       --min-aligned INT        leave out alignments with fewer aligned bases (CIGAR M + = + X)\n"
                 "       --min-identity FLOAT     leave out alignments whose identity 1 - NM / (M + = + X + I + D) is below FLOAT, in\n"
                 "                                [0, 1] (rounded to per-mille), or that carry no NM tag\n"
                 "       --device N | --devices N,M,... [--split-input] | --query-grouped | --any-order | --dump-records | --dump-raw\n"
                 "       --devices N,M,... --file-per-device   every listed device (one may be listed twice) is a slot that takes whole\n"
                 "                                     files of a directory, one at a time; the outputs are those of --device N\n"
                 "       --host-decode | --packed-records | --verify-grouping | --device-inflate K | --window-mb N |\n"
                 "       --decode-threads N | --no-mmap     (SLIMM_TRACE=cli: stage marks on stderr)\n"
                 "       --propagation-walk default|reversed   order in which the directly counted taxa hand their read counts up\n"
                 "                                     (default: lower ranks first, then ascending taxid; a [WARNING] names\n"
                 "                                     the taxa when a file's counts depend on it)\n";
}

// an unsigned number in [0, max], decimal or -- hex_too -- 0x...; nothing else in the text
bool parse_unsigned(const std::string& v, bool hex_too, uint64_t max, uint32_t& out) {
    const bool hex = hex_too && v.size() > 2 && v[0] == '0' && (v[1] == 'x' || v[1] == 'X');
    const size_t from = hex ? 2 : 0;
    if (v.size() == from || v.size() > from + 12) return false;
    for (size_t i = from; i < v.size(); ++i)
        if (!(hex ? isxdigit(static_cast<unsigned char>(v[i])) : isdigit(static_cast<unsigned char>(v[i])))) return false;
    const uint64_t n = strtoull(v.c_str() + from, nullptr, hex ? 16 : 10);
    if (n > max) return false;
    out = static_cast<uint32_t>(n);
    return true;
}

// 0 ok, 1 error, 2 help
int parse(int argc, char** argv, Options& o) {
    std::vector<std::string> pos;
    bool have_prefix = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto value = [&](std::string& dst) {
            if (i + 1 >= argc) {
                std::cerr << "slimm: option " << a << " needs a value\n";
                return false;
            }
            dst = argv[++i];
            return true;
        };
        std::string v;
        if (a == "-h" || a == "--help") {
            usage();
            return 2;
        } else if (a == "-o" || a == "--output-prefix") {
            if (!value(o.output_prefix)) return 1;
            have_prefix = true;
        } else if (a == "-w" || a == "--bin-width") {
            if (!value(v)) return 1;
            o.bin_width = static_cast<uint32_t>(strtoul(v.c_str(), nullptr, 10));
        } else if (a == "-mr" || a == "--min-reads") {
            if (!value(v)) return 1;
            o.min_reads = static_cast<uint32_t>(strtoul(v.c_str(), nullptr, 10));
        } else if (a == "-r" || a == "--rank") {
            if (!value(o.rank)) return 1;
            if (std::find_if(std::begin(kRankList), std::end(kRankList), [&](const char* r) { return o.rank == r; }) ==
                std::end(kRankList)) {
                std::cerr << "slimm: invalid rank '" << o.rank << "'\n";
                return 1;
            }
        } else if (a == "-cc" || a == "--cov-cut-off") {
            if (!value(v)) return 1;
            double d = strtod(v.c_str(), nullptr);
            if (d < 0.0 || d > 1.0) {
                std::cerr << "slimm: cov-cut-off must be in [0, 1]\n";
                return 1;
            }
            o.cov_cut_off = static_cast<float>(d);
        } else if (a == "-ac" || a == "--abundance-cut-off") {
            if (!value(v)) return 1;
            double d = strtod(v.c_str(), nullptr);
            if (d < 0.0 || d > 10.0) {
                std::cerr << "slimm: abundance-cut-off must be in [0, 10]\n";
                return 1;
            }
            o.abundance_cut_off = static_cast<float>(d);
        } else if (a == "-d" || a == "--directory") {
            o.is_directory = true;
        } else if (a == "-ro" || a == "--raw-output") {
            o.raw_output = true;
        } else if (a == "-co" || a == "--coverage-output") {
            o.coverage_output = true;
        } else if (a == "-v" || a == "--verbose") {
            o.verbose = true;
        } else if (a == "--devices") {
            if (!value(v)) return 1;
            o.devices.clear();
            for (size_t p = 0; p <= v.size();) {
                const size_t q = std::min(v.find(',', p), v.size());
                if (q > p) o.devices.push_back(atoi(v.substr(p, q - p).c_str()));
                p = q + 1;
            }
            if (!o.devices.empty()) o.device = o.devices[0];
        } else if (a == "--split-input") {
            o.split_input = true;
        } else if (a == "--file-per-device") {
            o.file_per_device = true;
        } else if (a == "--propagation-walk") {
            if (!value(v)) return 1;
            if (v != "default" && v != "reversed") {
                std::cerr << "slimm: propagation-walk must be default or reversed\n";
                return 1;
            }
            o.propagation_walk = v == "reversed" ? SLIMM_WALK_REVERSED : SLIMM_WALK_DEFAULT;
        } else if (a == "--device") {
            if (!value(v)) return 1;
            o.device = atoi(v.c_str());
        } else if (a == "--query-grouped") {
            o.order = SLIMM_ORDER_GROUPED;
        } else if (a == "--any-order") {
            o.order = SLIMM_ORDER_ANY;
        } else if (a == "--host-decode") {
            o.host_decode = true;
        } else if (a == "--packed-records") {
            o.packed_records = true;
        } else if (a == "--verify-grouping") {
            o.verify_grouping = true;
        } else if (a == "--device-inflate") {
            if (!value(v)) return 1;
            o.device_inflate = static_cast<unsigned>(std::max(0l, atol(v.c_str())));
        } else if (a == "--window-mb") {
            if (!value(v)) return 1;
            o.window_mb = static_cast<unsigned>(std::max(0l, atol(v.c_str())));
        } else if (a == "--decode-threads") {
            if (!value(v)) return 1;
            AlignmentFile::settings().threads = static_cast<unsigned>(std::max(1l, atol(v.c_str())));
        } else if (a == "--no-mmap") {
            AlignmentFile::settings().no_mmap = true;
        } else if (a == "-q" || a == "--min-mapq") {
            if (!value(v)) return 1;
            if (!parse_unsigned(v, false, 255, o.filter.min_mapq)) {
                std::cerr << "slimm: min-mapq must be an integer in [0, 255]\n";
                return 1;
            }
        } else if (a == "--require-flags" || a == "--exclude-flags") {
            if (!value(v)) return 1;
            if (!parse_unsigned(v, true, 0xffff, a == "--require-flags" ? o.filter.require_flags : o.filter.exclude_flags)) {
                std::cerr << "slimm: " << a.substr(2) << " must be a flag mask in [0, 65535], decimal or 0x...\n";
                return 1;
            }
        } else if (a == "--min-aligned") {
            if (!value(v)) return 1;
            if (!parse_unsigned(v, false, 0xffffffffull, o.filter.min_aligned)) {
                std::cerr << "slimm: min-aligned must be a number of bases, 0 or more\n";
                return 1;
            }
        } else if (a == "--min-identity") {
            if (!value(v)) return 1;
            char* rest = nullptr;
            const double d = strtod(v.c_str(), &rest);
            if (v.empty() || *rest || !(d >= 0.0 && d <= 1.0)) {
                std::cerr << "slimm: min-identity must be in [0, 1]\n";
                return 1;
            }
            o.filter.min_identity_permille = static_cast<uint32_t>(d * 1000.0 + 0.5);
        } else if (a == "--dump-records") {
            o.dump_records = true;
        } else if (a == "--dump-raw") {
            o.dump_records = o.dump_raw = true;
        } else if (!a.empty() && a[0] == '-' && a.size() > 1) {
            std::cerr << "slimm: unknown option " << a << "\n";
            return 1;
        } else {
            pos.push_back(a);
        }
    }
    if (o.file_per_device) {
        if (o.devices.empty()) {
            std::cerr << "slimm: --file-per-device needs --devices a,b,...: one slot per entry, each takes whole files\n";
            return 1;
        }
        if (o.split_input) {
            std::cerr << "slimm: --file-per-device and --split-input exclude each other: whole files on separate devices, or one file "
                         "over a group's members\n";
            return 1;
        }
        o.slots.swap(o.devices);
        o.device = o.slots[0];
    }
    if (o.dump_records && pos.size() == 1) {
        o.input_path = pos[0];
        return 0;
    }
    if (pos.size() != 2) {
        usage();
        return 1;
    }
    o.database_path = pos[0];
    o.input_path = pos[1];
    if (o.database_path.size() < 5 || o.database_path.substr(o.database_path.size() - 5) != ".sldb") {
        std::cerr << "slimm: the database must be a .sldb file\n";
        return 1;
    }
    if (!have_prefix) o.output_prefix = o.input_path;  // src/slimm.cpp:175-177
    return 0;
}

// --dump-raw: what the device decoder is fed -- the inflated bytes behind the BAM header (the text behind the header of a
// compressed SAM file), in windows of --window-mb (default 1) MiB -- to stdout, the window sizes to stderr
int dump_raw(const Options& o) {
    AlignmentFile f;
    if (!f.open(o.input_path)) {
        std::cerr << f.error() << "\n";
        return 1;
    }
    const size_t cap = static_cast<size_t>(std::max(1u, o.window_mb)) << 20;
    std::vector<uint8_t> buf(cap);
    long n;
    while ((n = f.streamed() ? f.read_text(buf.data(), cap) : f.read_raw(buf.data(), cap)) > 0) {
        std::cerr << "window\t" << n << "\t" << (f.raw_exhausted() ? "last" : "more") << "\n";
        if (fwrite(buf.data(), 1, static_cast<size_t>(n), stdout) != static_cast<size_t>(n)) return 1;
    }
    if (n < 0) {
        std::cerr << f.error() << "\n";
        return 1;
    }
    return 0;
}

// the record filter's counts of a file, as its log line has them: judged, the four dropped counts, no_nm when there is one
std::string filter_stats_line(const uint64_t* st) {
    std::ostringstream line;
    line << "record filter: " << st[SLIMM_RF_N_JUDGED] << " judged; dropped: " << st[SLIMM_RF_N_FLAGS] << " by flags, " << st[SLIMM_RF_N_MAPQ]
         << " by MAPQ, " << st[SLIMM_RF_N_ALIGNED] << " by aligned length, " << st[SLIMM_RF_N_IDENTITY] << " by identity";
    if (st[SLIMM_RF_N_NO_NM]) line << " (" << st[SLIMM_RF_N_NO_NM] << " of them without NM)";
    return line.str();
}

int dump_records(const Options& o) {
    if (o.dump_raw) return dump_raw(o);
    AlignmentFile f;
    f.set_filter(o.filter);
    if (!f.open(o.input_path)) {
        std::cerr << f.error() << "\n";
        return 1;
    }
    std::cout << "#format\t" << (f.is_bam() ? "BAM" : "SAM") << "\torder\t" << static_cast<int>(f.sort_order()) << "\n";
    for (size_t i = 0; i < f.ref_names().size(); ++i) std::cout << "@\t" << f.ref_names()[i] << "\t" << f.ref_lengths()[i] << "\n";
    RecordBatch b;
    long n;
    while ((n = f.read_batch(b, 1 << 20, true)) > 0) {
        for (size_t i = 0; i < b.size(); ++i)
            std::cout << b.qname[i] << "\t" << b.flag[i] << "\t" << b.ref_id[i] << "\t" << b.begin_pos[i] << "\t" << b.l_seq[i]
                      << "\t" << b.read_key[i] << "\n";
        b.clear();
    }
    if (n < 0) {
        std::cerr << f.error() << "\n";
        return 1;
    }
    std::cerr << "#q18_regroup_needed\t" << (f.q18_regroup_needed() ? 1 : 0) << "\n";   // (reader tests)
    if (o.filtered()) std::cerr << "#" << filter_stats_line(f.filter_stats()) << "\n";
    return 0;
}

// What every file of a run reads: filled by main() before the first file, read-only from then on -- but for the zero lineages
// that set_up adds to db.ac_taxid (Q13), under db_mu: --file-per-device sets files up side by side.
struct Shared {
    SlimmDatabase db;
    std::shared_mutex db_mu;
    std::vector<std::string> input_paths;
};

// Where a file's stderr lines go: to std::cerr as they come, or -- --file-per-device -- into a block that is printed whole once
// the blocks of the files before it are out.  Only the thread that runs the file's stages writes here.  The [trace] marks go
// to stderr at once either way, from several threads; `head` starts them and names the file where files run side by side.
struct FileLog {
    bool collect = false;
    std::ostringstream block;
    std::string head = "[trace] ";
    std::ostream& out() { return collect ? static_cast<std::ostream&>(block) : std::cerr; }
};

// What the one `slimm` object of the reference keeps across files (Q8): the values that a file sets for the files behind it.
// A slot of --file-per-device works on a copy of its own, taken once no file can change them any more (settled).
struct Session {
    Options options;   // (bin_width and min_reads: 0 until a file sets them)
    float cc_cache = 0.0f, ucc_cache = 0.0f;  // src/slimm.hpp:155-156: never cleared by reset() (Q8)
    uint32_t total_hits = 0;
    Shared* shared = nullptr;
    FileLog* log = nullptr;   // the file at hand
    std::ostream& err() const { return log->out(); }
    const char* trace_head() const { return log->head.c_str(); }
    // No file behind this point changes a carried value, and none reads one that another file wrote: set_up takes the bin
    // width from a file only while it is 0, the library derives min_reads only while it is 0 (HostProfile::set_coverage_strided)
    // and computes a cut-off only while its cache is 0.0 and the quantile below 1.0 (HostProfile::coverage_cut_off,
    // uniq_coverage_cut_off); what slimm_get_cutoff_cache hands back is then what slimm_set_cutoff_cache was given.
    bool settled() const {
        return options.bin_width != 0 && options.min_reads != 0 && (options.cov_cut_off >= 1.0f || (cc_cache != 0.0f && ucc_cache != 0.0f));
    }
};

// What one reading of a file comes to
enum class Outcome {
    Done,
    Failed,              // (the reason is printed)
    ReadAgainAnyOrder,   // Q18 on a file read as a grouped one: the file goes through the any-order path instead
    MoreMembers,         // more records than the contexts of the group take (a group on one device: run_group)
};

#define CHECK(ctx, call)                                                            \
    do {                                                                            \
        if ((call) < 0) {                                                           \
            S.err() << "slimm: " << #call << ": " << slimm_last_error(ctx) << "\n";  \
            return Outcome::Failed;                                                 \
        }                                                                           \
    } while (0)

// the library's handles, destroyed when their owner goes
using CtxPtr = std::unique_ptr<slimm_ctx, void (*)(slimm_ctx*)>;
using GroupPtr = std::unique_ptr<slimm_group, void (*)(slimm_group*)>;

// the file's size: what the library sizes its window buffers by (include/slimm_hip.h, slimm_set_input_size_hint)
void set_size_hint(slimm_ctx* ctx, const std::string& path) {
    struct stat st;
    if (stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode)) (void)slimm_set_input_size_hint(ctx, static_cast<uint64_t>(st.st_size));
}

// the file from its first record again; false after printing why it could not be opened
bool reopen(AlignmentFile& bam, const std::string& path, std::ostream& err) {
    bam.close();
    if (bam.open(path)) return true;
    err << bam.error() << "\n";
    return false;
}

// The two failed pushes the command reacts to, told apart by the library's message (they share SLIMM_E_INVALID with every
// other failed push): a record longer than the device decoder's carry, and more records than one context takes.
enum class PushError { HostDecode, RecordCap, Other };
PushError classify(const char* message) {
    if (strstr(message, "decode this file on the host")) return PushError::HostDecode;
    if (strstr(message, "fewer than 2^31 records")) return PushError::RecordCap;
    return PushError::Other;
}

float depth_of(const uint32_t* bins, uint32_t n, uint32_t nz) {  // reference_contig.hpp:188-207 + misc.hpp:285-289
    if (nz == 0) return 0.0f;
    float s = 0.0f;
    for (uint32_t i = 0; i < n; ++i) s += float(bins[i]);
    return s / n;
}

// SLIMM_TRACE=cli: millisecond marks of the per-file stages on stderr (the reference's own timer prints whole seconds)
struct Trace {
    bool on = g_trace;
    std::string head = "[trace] ";   // (FileLog::head)
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "%s%-34s %9.2f ms\n", head.c_str(), what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// SLIMM_TRACE=cli: what the file's end holds -- device memory in use (hipMemGetInfo: everything on the device), the window
// pipeline's share of it, and the process's peak resident set
void trace_memory(slimm_ctx* ctx, const char* head) {
    uint64_t used = 0, total = 0, win = 0;
    (void)slimm_device_memory(ctx, &used, &total);
    (void)slimm_window_memory(ctx, &win);
    long hwm_kb = 0;
    if (FILE* f = fopen("/proc/self/status", "r")) {
        char line[256];
        while (fgets(line, sizeof line, f))
            if (sscanf(line, "VmHWM: %ld kB", &hwm_kb) == 1) break;
        fclose(f);
    }
    fprintf(stderr, "%sdevice memory in use %.2f GB of %.0f GB (window pipeline %.2f GB); host peak resident set %.2f GB\n", head, used / 1e9,
            total / 1e9, win / 1e9, hwm_kb / 1e6);
}

// Where a file's records go: one context, or a group that deals the decoded records to its members (ctx is then member 0,
// which takes the device decoders' bytes: slimm_group_get_profiles deals those records device to device afterwards).
struct Target {
    slimm_ctx* ctx = nullptr;
    slimm_group* group = nullptr;
    int push_checked(const uint64_t* key, const int32_t* ref, const int32_t* pos, const uint16_t* flag, const uint32_t* check,
                     uint64_t n) const {
        return group ? slimm_group_push_records_checked(group, key, ref, pos, flag, check, n)
                     : slimm_push_records_checked(ctx, key, ref, pos, flag, check, n);
    }
    int push_marked(const uint32_t* word, const int32_t* pos, uint64_t n) const {
        return group ? slimm_group_push_records_marked(group, word, pos, n) : slimm_push_records_marked(ctx, word, pos, n);
    }
    int push_packed(const uint64_t* key, const int32_t* ref, const int32_t* pos, uint64_t n) const {
        return group ? slimm_group_push_records_packed(group, key, ref, pos, n) : slimm_push_records_packed(ctx, key, ref, pos, n);
    }
    int reset() const { return group ? slimm_group_reset(group) : slimm_reset(ctx); }
    const char* error() const { return group ? slimm_group_last_error(group) : slimm_last_error(ctx); }
};

// THE FORMS OF AN INPUT FILE: one row per form says what the command's two readers of file bytes -- RecordPump's raw windows
// and read_split -- need to know of it.  A new form is a row.
struct InputForm {
    const char* name;   // in the [trace] lines (a streamed codec's: "a <name> stream", "<name> SAM on the device")
    const char* article = "a";   // ... and its article there
    bool sam;           // SAM text: the decoder wants the header's reference names first (slimm_set_reference_names)
    // Which AlignmentFile path supplies the pump's bytes.  Bgzf: read_blocks -- whole blocks, the device inflates them -- every
    // device_period-th window, else read_raw; `last` from raw_exhausted().  Text: read_text.  Streamed: read_compressed, the
    // file's bytes from its first on; the first push skips text_header_bytes() decoded bytes, `last` from compressed_exhausted()
    enum Read { Bgzf, Text, Streamed } read;
    // (ctx, bytes, n, skip, last, &got): a window of those bytes -- and the empty final push, (nullptr, 0, skip, 1), when the end
    // came without notice or a range is empty.  push_blocks: whole BGZF blocks as they lie in the file
    using Push = int (*)(slimm_ctx*, const uint8_t*, uint64_t, uint32_t, int, uint64_t*);
    Push push, push_blocks = nullptr;
    // --split-input and the re-read at the record cap: the planner of the members' byte ranges (none: the form is never cut),
    // and what read_split says it plans: "the file's <planned> could not be planned into ranges"
    int (*plan)(const char* path, uint64_t header_bytes, uint32_t n, uint64_t* offsets) = nullptr;
    const char* planned = nullptr;
    bool header_32bit = true;          // ... only with a header of fewer than 2^32 inflated bytes (member 0's `skip`)
    bool wide_header_by_host = false;  // the pump: a header of 2^32 text bytes or more goes through the host reader (pushed_as)
    uint64_t (*slack)() = nullptr;     // bytes a member reads behind its range, at most to the file's end (none: 0)
    bool announce_range = false;       // the members are told their ranges (slimm_set_input_range)
    // gzip: the plan's offsets are BITS -- a member reads the bytes that hold its bits and is told the bits --, and every
    // member but the last reads its range twice: the window pass (window_pass(ctx, 1)), then windows(group), then the text pass
    int (*announce_bits)(slimm_ctx*, uint64_t begin_bit, uint64_t end_bit) = nullptr;
    int (*window_pass)(slimm_ctx*, int on) = nullptr;
    int (*windows)(slimm_group*) = nullptr;
    // ... and what a range that starts at `offset` cannot see of the file in front of it, beside its range (none: nothing)
    int (*range_note)(const char* path, uint64_t offset, int* note) = nullptr;
    int (*announce_note)(slimm_ctx*, int note) = nullptr;
    // what else must hold for a regular file of this form to be cut over G members (cut_by_byte_range; none: nothing).  The
    // least units -- bytes or blocks -- a member is worth; how many lie behind the header's last frame, block or bit (false:
    // the file is not cut); units_gate: that answer is a condition of its own, asked without the floor too
    uint64_t (*split_floor)() = nullptr;
    bool (*units_behind)(const std::string& path, uint64_t header_bytes, uint64_t* units) = nullptr;
    bool units_gate = false;
    // SLIMM_TRACE=cli, at the file's end: what the device decoded, the counters of the n contexts summed (none: no line)
    void (*end_line)(const char* head, slimm_ctx* const* ctx, uint32_t n) = nullptr;
    // a regular file of this form that the host reader takes all the same, and says so under SLIMM_TRACE=cli (none: never)
    bool (*by_host)(const std::string& path, const char* head) = nullptr;
};
int push_sam_text(slimm_ctx* c, const uint8_t* p, uint64_t n, uint32_t, int last, uint64_t* got) { return slimm_push_sam_bytes(c, p, n, last, got); }
int push_bam_records(slimm_ctx* c, const uint8_t* p, uint64_t n, uint32_t, int last, uint64_t* got) { return slimm_push_bam_bytes(c, p, n, last, got); }

// bytes [at, at + n) of the file into dst; false on a read error or a short file
bool pread_all(int fd, uint8_t* dst, uint64_t at, size_t n) {
    for (; n;) {
        const ssize_t k = pread(fd, dst, n, static_cast<off_t>(at));
        if (k <= 0) return false;
        dst += k, at += static_cast<uint64_t>(k), n -= static_cast<size_t>(k);
    }
    return true;
}
void gzip_end_line(const char* head, slimm_ctx* const* ctx, uint32_t n) {
    uint64_t members = 0, chunks = 0, dropped = 0, text = 0, told = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t st[20] = {};
        if (slimm_get_gzip_stats(ctx[i], st) == SLIMM_OK) ++told, members += st[0], chunks += st[1], dropped += st[3], text += st[9];
    }
    if (told) fprintf(stderr, "%sgzip SAM on the device: %llu members, %llu chunks (%llu candidates dropped), %llu bytes of text\n", head,
            (unsigned long long)members, (unsigned long long)chunks, (unsigned long long)dropped, (unsigned long long)text);
}
void zstd_end_line(const char* head, slimm_ctx* const* ctx, uint32_t n) {
    uint64_t frames = 0, blocks = 0, text = 0, told = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t st[20] = {};
        if (slimm_get_zstd_stats(ctx[i], st) == SLIMM_OK) ++told, frames += st[0], blocks += st[2] + st[3] + st[4], text += st[16];
    }
    if (told) fprintf(stderr, "%szstd SAM on the device: %llu frames, %llu blocks, %llu bytes of text\n", head, (unsigned long long)frames,
            (unsigned long long)blocks, (unsigned long long)text);
}
void lz4_end_line(const char* head, slimm_ctx* const* ctx, uint32_t n) {
    uint64_t frames = 0, blocks = 0, text = 0, told = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t st[20] = {};
        if (slimm_get_lz4_stats(ctx[i], st) == SLIMM_OK) ++told, frames += st[0], blocks += st[3] + st[4], text += st[9];
    }
    if (told) fprintf(stderr, "%slz4 SAM on the device: %llu frames, %llu blocks, %llu bytes of text\n", head, (unsigned long long)frames,
            (unsigned long long)blocks, (unsigned long long)text);
}
void xz_end_line(const char* head, slimm_ctx* const* ctx, uint32_t n) {
    uint64_t streams = 0, blocks = 0, text = 0, told = 0;
    for (uint32_t i = 0; i < n; ++i) {   // (a stream is counted by the member that read its header)
        uint64_t st[20] = {};
        if (slimm_get_xz_stats(ctx[i], st) == SLIMM_OK) ++told, streams += st[0], blocks += st[1], text += st[14];
    }
    if (told) fprintf(stderr, "%sxz SAM on the device: %llu streams, %llu blocks, %llu bytes of text\n", head, (unsigned long long)streams,
            (unsigned long long)blocks, (unsigned long long)text);
}
// xz SAM is decoded a lane per block, so a file of few blocks would keep few lanes busy for a long time: the command reads
// the file's index or indexes from its end (xz_read_index) and takes the device path only for kXzDeviceBlocks blocks or more
// -- a stated default, not a measurement (SLIMM_FORCE xz_device_blocks=N).  A file whose index does not parse goes by the
// host reader as well, which says what is wrong with it
constexpr uint64_t kXzDeviceBlocks = 16;
uint64_t xz_device_blocks() { return forced_or("xz_device_blocks", kXzDeviceBlocks); }
// (one reading of a file's indexes for the two questions below; false: not a file whose index parses)
bool xz_index_of(const std::string& path, uint64_t* size, std::vector<XzIndexBlock>* blocks, std::vector<XzIndexStream>* layout) {
    const int fd = open(path.c_str(), O_RDONLY);
    struct stat sb;
    uint32_t streams = 0;
    const bool ok = fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) &&
                    xz_read_index([&](uint64_t at, uint8_t* dst, size_t n) { return pread_all(fd, dst, at, n); }, static_cast<uint64_t>(sb.st_size), blocks, &streams, layout);
    if (fd >= 0) close(fd);
    if (ok) *size = static_cast<uint64_t>(sb.st_size);
    return ok;
}
bool xz_by_host(const std::string& path, const char* head) {
    uint64_t size = 0;
    std::vector<XzIndexBlock> blocks;
    const bool ok = xz_index_of(path, &size, &blocks, nullptr);
    if (ok && blocks.size() >= xz_device_blocks()) return false;
    if (g_trace && ok) fprintf(stderr, "%sxz SAM of %llu block(s): read on the host\n", head, (unsigned long long)blocks.size());
    if (g_trace && !ok) fprintf(stderr, "%sxz SAM whose index does not parse: read on the host\n", head);
    return true;
}
// What the forms with a floor count for cut_by_byte_range.  The floors are stated defaults, not measurements: zstd's is the
// codec's round size, gzip's is zstd's (a range is decoded twice, so two members may not gain), xz's is kXzDeviceBlocks (a
// range is decoded a lane per block, as a file is).  zstd, gzip: the bytes behind the first legal cut
bool zstd_bytes_behind(const std::string& path, uint64_t header_bytes, uint64_t* bytes) {
    PlanFile f;
    uint64_t first = 0;
    if (!f.open_regular(path.c_str()) || !zstd_header_end(f.reader(), f.size, header_bytes, &first) || first > f.size) return false;
    *bytes = f.size - first;
    return true;
}
bool gzip_bytes_behind(const std::string& path, uint64_t header_bytes, uint64_t* bytes) {
    PlanFile f;
    uint64_t first_bit = 0;
    if (!f.open_regular(path.c_str()) || !slimm::gzip_header_end(f.reader(), f.size, header_bytes, &first_bit)) return false;
    *bytes = f.size - first_bit / 8u;
    return true;
}
// xz: the blocks behind those that hold the header, which are member 0's in any case.  Whether the device reads the file at
// all is xz_by_host's to say, and set_up asks it only behind this: so a file of fewer than xz_device_blocks() blocks -- the one
// threshold, asked here as xz_by_host asks it -- is not cut, --split-input leaves it to member 0's host reader, and at the
// cap, where the host reader has read it, it fails as it did
bool xz_blocks_behind(const std::string& path, uint64_t header_bytes, uint64_t* behind) {
    uint64_t size = 0, text = 0;
    std::vector<XzIndexBlock> blocks;
    if (!xz_index_of(path, &size, &blocks, nullptr) || blocks.size() < xz_device_blocks()) return false;
    *behind = blocks.size();
    for (const XzIndexBlock& b : blocks) {
        if (text >= header_bytes) break;
        text += b.uncompressed;
        --*behind;
    }
    return true;
}

// lzip SAM is decoded a lane per member, as xz a lane per block: the command counts the file's members by their trailers
// (slimm_host_lzip_members) and takes the device path only for kLzipDeviceMembers members or more -- xz's 16, the project's own
// stated default, not a measurement (SLIMM_FORCE lzip_device_members=N).  A file whose trailers do not chain to its first byte
// goes by the host reader as well, which says what is wrong with it
constexpr uint64_t kLzipDeviceMembers = 16;
uint64_t lzip_device_members() { return forced_or("lzip_device_members", kLzipDeviceMembers); }
bool lzip_by_host(const std::string& path, const char* head) {
    uint64_t members = 0, text = 0;
    const bool ok = slimm_host_lzip_members(path.c_str(), &members, &text) == SLIMM_OK;
    if (ok && members >= lzip_device_members()) return false;
    if (g_trace && ok) fprintf(stderr, "%slzip SAM of %llu member(s): read on the host\n", head, (unsigned long long)members);
    if (g_trace && !ok) fprintf(stderr, "%slzip SAM whose trailers do not chain to its first byte: read on the host\n", head);
    return true;
}
void lzip_end_line(const char* head, slimm_ctx* const* ctx, uint32_t n) {
    uint64_t members = 0, text = 0, told = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t st[20] = {};
        if (slimm_get_lzip_stats(ctx[i], st) == SLIMM_OK) ++told, members += st[0], text += st[7];
    }
    if (told) fprintf(stderr, "%slzip SAM on the device: %llu members, %llu bytes of text\n", head, (unsigned long long)members, (unsigned long long)text);
}

enum { kBam, kBgzfSam, kSam, kBzip2Sam, kGzipSam, kZstdSam, kXzSam, kLz4Sam, kLzipSam };
const InputForm kForms[] = {
    {.name = "BAM", .sam = false, .read = InputForm::Bgzf, .push = push_bam_records, .push_blocks = slimm_push_bgzf_blocks,
     .plan = slimm_host_bgzf_ranges, .planned = "BGZF blocks"},
    {.name = "BGZF SAM", .sam = true, .read = InputForm::Bgzf, .push = push_sam_text, .push_blocks = slimm_push_bgzf_sam_blocks,
     .plan = slimm_host_bgzf_ranges, .planned = "BGZF blocks"},
    {.name = "SAM", .sam = true, .read = InputForm::Text, .push = push_sam_text, .plan = slimm_host_text_ranges, .planned = "text", .header_32bit = false},
    {.name = "bzip2", .sam = true, .read = InputForm::Streamed, .push = slimm_push_bzip2_sam_bytes, .plan = slimm_host_bzip2_ranges,
     .planned = "bzip2 streams", .slack = slimm_bzip2_split_slack, .announce_range = true},
    {.name = "gzip", .sam = true, .read = InputForm::Streamed, .push = slimm_push_gzip_sam_bytes, .plan = slimm_host_gzip_ranges,
     .planned = "gzip blocks", .wide_header_by_host = true, .announce_bits = slimm_set_gzip_range, .window_pass = slimm_set_gzip_window_pass,
     .windows = slimm_group_gzip_windows, .split_floor = slimm_gzip_split_floor, .units_behind = gzip_bytes_behind, .end_line = gzip_end_line},
    {.name = "zstd", .sam = true, .read = InputForm::Streamed, .push = slimm_push_zstd_sam_bytes, .plan = slimm_host_zstd_ranges,
     .planned = "zstd frames", .wide_header_by_host = true, .announce_range = true, .split_floor = slimm_zstd_split_floor,
     .units_behind = zstd_bytes_behind, .end_line = zstd_end_line},
    {.name = "xz", .article = "an", .sam = true, .read = InputForm::Streamed, .push = slimm_push_xz_sam_bytes, .plan = slimm_host_xz_ranges,
     .planned = "xz blocks", .wide_header_by_host = true, .announce_range = true, .range_note = slimm_host_xz_check_at,
     .announce_note = slimm_set_xz_range_check, .split_floor = slimm_xz_split_floor, .units_behind = xz_blocks_behind, .units_gate = true,
     .end_line = xz_end_line, .by_host = xz_by_host},
    // (no planner: an lz4 file goes through member 0's decoder whole, and --split-input leaves it there)
    {.name = "lz4", .article = "an", .sam = true, .read = InputForm::Streamed, .push = slimm_push_lz4_sam_bytes, .wide_header_by_host = true,
     .end_line = lz4_end_line},
    // (no planner either: the cut at member starts, found from the trailers, is not built)
    {.name = "lzip", .article = "an", .sam = true, .read = InputForm::Streamed, .push = slimm_push_lzip_sam_bytes, .wide_header_by_host = true,
     .end_line = lzip_end_line, .by_host = lzip_by_host},
};
const InputForm& form_of(const AlignmentFile& f) {
    if (f.is_bam()) return kForms[kBam];
    switch (f.compression()) {
        case Compression::Bgzf: return kForms[kBgzfSam];
        case Compression::Bzip2: return kForms[kBzip2Sam];
        case Compression::Gzip: return kForms[kGzipSam];
        case Compression::Zstd: return kForms[kZstdSam];
        case Compression::Xz: return kForms[kXzSam];
        case Compression::Lz4: return kForms[kLz4Sam];
        case Compression::Lzip: return kForms[kLzipSam];
        default: return kForms[kSam];
    }
}
// What RecordPump's raw windows push a file as: its own form -- but where the row says so (gzip, zstd, xz) a header of 2^32 text
// bytes or more goes through the host reader (the push's `skip` has 32 bits): read_text decodes it, and the text is plain SAM's
const InputForm& pushed_as(const AlignmentFile& f) {
    const InputForm& form = form_of(f);
    return form.wide_header_by_host && f.text_header_bytes() >= (1ull << 32) ? kForms[kSam] : form;
}
// ... and whether it has raw windows at all: SAM text from anything but a regular file -- a pipe -- goes through the host
// decoder's buffered reads
bool has_raw_windows(const AlignmentFile& f) { return f.is_bam() || f.regular_file(); }
// The header's length as a form's planner and its member 0 count it: a streamed codec's in decoded text bytes (for gzip
// header_bytes() does not say them; for the others the two are one number)
uint64_t planned_header_bytes(const InputForm& form, const AlignmentFile& f) {
    return form.read == InputForm::Streamed ? f.text_header_bytes() : f.header_bytes();
}
// A file's plan for G members: G + 1 offsets (false: the form has no planner, the header is too long for it, or it failed)
bool plan_ranges(const InputForm& form, const std::string& path, uint64_t header_bytes, uint32_t G, std::vector<uint64_t>& off) {
    off.assign(G + 1u, 0);
    return form.plan && !(form.header_32bit && header_bytes >= (1ull << 32)) && form.plan(path.c_str(), header_bytes, G, off.data()) == SLIMM_OK;
}
// The files read_split takes: regular files of a form that has a planner.  A form with a floor (gzip, zstd, xz) is cut only for
// two members or more, with a header of fewer than 2^32 bytes, where -- with_floor -- the units behind the first legal cut,
// divided by G, reach the floor (the cap's re-read does not ask: it has no other way; asked first: the plan reads more of the
// file), and where the plan leaves at least two ranges that are not empty (a zstd file of one frame has none).  *planned
// keeps that plan's G + 1 offsets for read_split (empty: not cut, or a form without a floor, which read_split plans)
bool cut_by_byte_range(const AlignmentFile& f, const std::string& path, uint32_t G, bool with_floor, std::vector<uint64_t>* planned) {
    const InputForm& form = form_of(f);
    planned->clear();
    if (!f.regular_file() || !form.plan) return false;
    if (!form.split_floor) return true;
    const uint64_t header_bytes = planned_header_bytes(form, f);
    if (G < 2u || header_bytes >= (1ull << 32)) return false;
    uint64_t units = 0, filled = 0;
    if ((with_floor || form.units_gate) && !form.units_behind(path, header_bytes, &units)) return false;
    if (with_floor && units / G < form.split_floor()) return false;
    if (plan_ranges(form, path, header_bytes, G, *planned))
        for (uint32_t i = 0; i < G; ++i) filled += (*planned)[i + 1] > (*planned)[i] ? 1u : 0u;
    if (filled < 2u) planned->clear();
    return filled >= 2u;
}
// One window of a file's bytes to the device decoder of its form; n = 0: the empty final push
int push_window(const InputForm& form, slimm_ctx* ctx, const uint8_t* bytes, uint64_t n, bool compressed, uint32_t skip, bool last, uint64_t* got) {
    if (!n) return form.push(ctx, nullptr, 0, skip, 1, got);
    return (compressed && form.push_blocks ? form.push_blocks : form.push)(ctx, bytes, n, skip, last ? 1 : 0, got);
}
// A push is one device window at most: what its bytes may inflate to, for a window buffer of `cap` bytes (SAM text in BGZF
// blocks may compress 24-fold: 80 MB of blocks fill it)
size_t max_inflated_per_push(size_t cap) { return std::min<size_t>(10 * cap, 1900u << 20); }

// The record stream of one file, decoded on a thread of its own from the moment the file is open: while the main thread
// builds the lineage table and creates the context (the HIP runtime's start-up included), batches pile up in host
// memory; once the context exists they are pushed in order and the decoder switches to the context's page-locked
// staging sets, which the DMA engine reads while the next batch is decoded (slimm_push_staged_async).
struct RecordPump {
    static constexpr uint64_t kBatch = 1 << 20;   // records per batch
    static constexpr size_t kMaxQueued = 64;      // batches held in host memory before the decoder waits for the context
    struct Batch {
        std::unique_ptr<uint64_t[]> key{new uint64_t[kBatch]};
        std::unique_ptr<int32_t[]> ref{new int32_t[kBatch]}, pos{new int32_t[kBatch]};
        std::unique_ptr<uint16_t[]> flag{new uint16_t[kBatch]};
        std::unique_ptr<uint32_t[]> check;  // only for streams in no particular order (want_check)
        uint64_t n = 0;
    };
    AlignmentFile& bam;
    // want_check: the stream is in no particular order, so two read names with one key would meet after the device sort
    // unnoticed -- every record then carries a second hash of its name (slimm_push_records_checked; no staging sets)
    const bool want_check;
    // Name-grouped input (no check words) goes over the bus as RUN-MARKED 8-byte records: the reader has made the keys of
    // adjacent records equal exactly when their names are, so "this record starts a qName run" is a key comparison on the
    // host and the device never sees a key (include/slimm_hip.h, slimm_mark_word).  --verify-grouping needs the keys
    // on the device and keeps the packed 16-byte form; so does --packed-records.
    const bool marked;
    uint64_t last_key = 0;   // the key of the last record marked so far (batches are pushed in file order)
    bool have_last = false;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Batch> queued;
    Target target;             // set by drain(): from then on the decoder pushes by itself
    bool failed = false;       // a push failed (slimm_last_error says why)
    long read_rc = 0;          // the reader's last answer: 0 = end of file, -1 = format error
    double decode_ms = 0, wait_ms = 0;
    std::thread th;

    // DEVICE DECODE (BAM files, one context): the decoder thread only inflates -- windows of BGZF-inflated record bytes
    // go into a few large host buffers, a second thread hands them to slimm_push_bam_bytes, and the device finds the
    // record boundaries, reads the fields and compares / hashes the names (slimm_amd/csrc/bam_decode.hip).  The host
    // walked every inflated byte three times for that.  --host-decode keeps the host decoder.
    const bool raw;
    const InputForm& form;    // what the raw windows are read and pushed as
    const std::string head;   // what the [trace] lines start with (FileLog::head)
    // bytes per window buffer (--window-mb: tests make windows smaller than a record)
    static size_t& raw_cap_setting() {
        static size_t cap = 192u << 20;
        return cap;
    }
    static size_t raw_cap() { return raw_cap_setting(); }
    static constexpr unsigned kRawBuffers = 4;
    struct RawWindow {
        unsigned which = 0;
        long n = 0;          // bytes; 0 = end of file, -1 = the reader failed
        bool last = false;   // the reader knows that nothing follows
        bool compressed = false;  // the bytes are whole BGZF blocks as they lie in the file: the device inflates them
    };
    // The windows the reader takes straight from the file are handed over COMPRESSED (slimm_push_bgzf_blocks): 192 MB of
    // BGZF blocks at a time, read by pread on several threads; the library gathers them into device windows of 1.4 - 1.9 GB
    // of inflated bytes (its inflater's first phase is a lane per block and wants tens of thousands of blocks) and inflates
    // them in two phases on two streams in turn (slimm_amd/csrc/bgzf_tokens.hip) while the next windows cross the bus.
    // --device-inflate k: every k-th of those windows only, the others inflated by the host cores (0 = all on
    // the host: rounds 1 - 3; 6 = round 4's default, when the device inflated 19 - 38 GB/s and 16 host cores 14 - 55).
    // Measured on 100 M records that compress 3-fold (scripts/realistic_cli.py): host inflate 2.1 - 2.3 s, this 0.7 s.
    unsigned device_period = 1;
    size_t device_window = 0;  // inflated bytes of a device window
    uint64_t raw_windows_device = 0, raw_windows_host = 0;
    // (mapped with MADV_HUGEPAGE where the kernel grants it: 192 MB in 4 KB pages are 49 K page faults to fill and as many
    // pages to give back when the process leaves -- a quarter second of a one-second run over the four buffers)
    struct RawUnmap {
        void operator()(uint8_t* p) const {
            if (p) munmap(p, raw_cap());
        }
    };
    std::unique_ptr<uint8_t, RawUnmap> raw_buf[kRawBuffers];
    static uint8_t* raw_map() {
        void* p = mmap(nullptr, raw_cap(), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return nullptr;
        (void)madvise(p, raw_cap(), MADV_HUGEPAGE);
        return static_cast<uint8_t*>(p);
    }
    std::deque<RawWindow> raw_ready;   // inflated, waiting to be pushed
    unsigned raw_free = kRawBuffers;
    std::thread raw_pusher;
    uint64_t raw_records = 0;
    double raw_push_ms = 0;

    RecordPump(AlignmentFile& f, bool check_words, bool device_decode, const Options& o, const std::string& trace_head)
        : bam(f), want_check(check_words),
          marked(!check_words && !o.verify_grouping && !o.packed_records),
          raw(device_decode && !o.verify_grouping && !o.packed_records && !o.host_decode && has_raw_windows(f)),
          form(pushed_as(f)), head(trace_head) {
        device_period = o.device_inflate;
        device_window = max_inflated_per_push(raw_cap());
        th = std::thread([this] { raw ? run_raw() : run(); });  // (in the body: every member is initialised by now)
    }
    ~RecordPump() {
        if (th.joinable() || raw_pusher.joinable()) {
            {
                std::lock_guard<std::mutex> g(mu);
                failed = true;  // (an early return of the caller: let the decoder out of its wait)
            }
            cv.notify_all();
            if (th.joinable()) th.join();
            if (raw_pusher.joinable()) raw_pusher.join();
        }
    }
    // the inflater of the device-decode mode: fills the window buffers in turn.  BGZF files -- BAM, or SAM text -- alike:
    // windows the host inflates (read_raw) and, every device_period-th of those read in place, whole blocks (read_blocks)
    void run_raw() {
        for (unsigned w = 0;; w = (w + 1) % kRawBuffers) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return failed || raw_free > 0; });
                if (failed) return;
                --raw_free;
            }
            if (!raw_buf[w]) raw_buf[w].reset(raw_map());
            if (!raw_buf[w]) {
                std::lock_guard<std::mutex> g(mu);
                failed = true;
                cv.notify_all();
                return;
            }
            auto t1 = std::chrono::steady_clock::now();
            // (every device_period-th of the windows read in place)
            bool compressed = false;
            long n;
            if (form.read == InputForm::Streamed) {   // the file's bytes as they lie in it (the codec's push decodes them)
                n = bam.read_compressed(raw_buf[w].get(), raw_cap());
                compressed = true;
                ++raw_windows_device;
            } else if (form.read == InputForm::Text) {   // SAM, plain: the text (slimm_push_sam_bytes finds and decodes the lines)
                n = bam.read_text(raw_buf[w].get(), raw_cap());
                ++raw_windows_device;
            } else if (device_period && bam.can_read_blocks() && (raw_windows_device + raw_windows_host) % device_period == device_period - 1u) {
                size_t inflated = 0;
                n = bam.read_blocks(raw_buf[w].get(), raw_cap(), device_window, &inflated);
                compressed = true;
                ++raw_windows_device;
            } else {
                n = bam.read_raw(raw_buf[w].get(), raw_cap());
                if (bam.can_read_blocks() || bam.raw_exhausted()) ++raw_windows_host;
            }
            decode_ms += ms(t1, std::chrono::steady_clock::now());
            {
                std::lock_guard<std::mutex> g(mu);
                raw_ready.push_back(RawWindow{w, n, n > 0 && (form.read == InputForm::Streamed ? bam.compressed_exhausted() : form.read == InputForm::Bgzf && bam.raw_exhausted()), compressed});
            }
            cv.notify_all();
            if (n <= 0) {
                read_rc = n;
                return;
            }
        }
    }
    // ... and the thread that hands them to the device, from the moment the context exists
    void push_raw(slimm_ctx* c) {
        bool pinned[kRawBuffers] = {};
        bool closed = false;  // a window went out as the file's last
        bool in_flight = false;  // the window pushed last is still being copied out of its buffer
        bool end_traced = false;
        // (a streamed file goes from its first byte: the first push skips the header's decoded bytes)
        uint32_t skip = form.read == InputForm::Streamed ? static_cast<uint32_t>(bam.text_header_bytes()) : 0u;
        if (form.sam) {   // SAM text names its references: the header's names for the device's look-up
            std::vector<const char*> names;
            for (const std::string& nm : bam.ref_names()) names.push_back(nm.c_str());
            if (slimm_set_reference_names(c, names.data()) != SLIMM_OK) {
                std::lock_guard<std::mutex> g(mu);
                failed = true;
                cv.notify_all();
                return;
            }
        }
        for (;;) {
            RawWindow w;
            {
                std::unique_lock<std::mutex> g(mu);
                auto t0 = std::chrono::steady_clock::now();
                cv.wait(g, [&] { return failed || !raw_ready.empty(); });
                wait_ms += ms(t0, std::chrono::steady_clock::now());
                if (failed) return;
                w = raw_ready.front();
                raw_ready.pop_front();
            }
            if (w.n < 0) return;  // (the reader failed: read_rc says so)
            int rc = SLIMM_OK;
            uint64_t got = 0;
            auto t1 = std::chrono::steady_clock::now();
            if (w.n > 0) {
                if (!pinned[w.which]) {
                    (void)slimm_pin_host_buffer(c, raw_buf[w.which].get(), raw_cap());  // (pageable memory still works)
                    pinned[w.which] = true;
                }
                rc = push_window(form, c, raw_buf[w.which].get(), static_cast<uint64_t>(w.n), w.compressed, skip, w.last, &got);
                skip = 0;
                closed = w.last;
            } else if (!closed) {
                rc = push_window(form, c, nullptr, 0, false, skip, true, &got);  // (the end came without notice: an incomplete record is an error)
            }
            raw_push_ms += ms(t1, std::chrono::steady_clock::now());
            raw_records += got;
            if (form.end_line && g_trace && rc >= 0 && (closed || w.n == 0) && !end_traced) {   // (the file's end: what the device decoded)
                end_traced = true;
                form.end_line(head.c_str(), &c, 1);
            }
            {
                // (a window's buffer is the library's until the NEXT push returns: its copy runs beside the work on the
                // window before it)
                std::lock_guard<std::mutex> g(mu);
                if (in_flight) ++raw_free;
                in_flight = w.n > 0 && !closed;
                if (w.n > 0 && closed) ++raw_free;
                if (w.n == 0) ++raw_free;
                if (rc < 0) failed = true;
            }
            cv.notify_all();
            if (rc < 0 || w.n == 0) return;
        }
    }
    // 16 bytes per record over the bus: the three flag bits the path reads go into the key's top bits
    // (include/slimm_hip.h, slimm_pack_key); every unchecked push of a file is packed -- the forms do not mix
    static void pack(uint64_t* key, const uint16_t* flag, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t f = flag[i];
            const uint64_t mate = (f & 0x40u) ? 1u : ((f & 0x80u) ? 2u : 0u);
            key[i] = (key[i] & ((1ull << 61) - 1ull)) | (mate << 61) | (((f >> 2) & 1ull) << 63);
        }
    }
    // in place: ref[] becomes the words {reference + 1 | mate << 29 | starts a run << 31}
    uint32_t* mark(const uint64_t* key, const uint16_t* flag, int32_t* ref, uint64_t n) {
        uint32_t* word = reinterpret_cast<uint32_t*>(ref);
        slimm_mark_words(key, flag, ref, n, have_last ? &last_key : nullptr, word);
        last_key = key[n - 1];
        have_last = true;
        return word;
    }
    int push(Batch& b) {
        if (b.check) return target.push_checked(b.key.get(), b.ref.get(), b.pos.get(), b.flag.get(), b.check.get(), b.n);
        if (marked) return target.push_marked(mark(b.key.get(), b.flag.get(), b.ref.get(), b.n), b.pos.get(), b.n);
        pack(b.key.get(), b.flag.get(), b.n);
        return target.push_packed(b.key.get(), b.ref.get(), b.pos.get(), b.n);
    }
    static double ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    }
    void run() {
        uint32_t which = 0;
        for (;;) {
            slimm_ctx* c;
            {
                std::lock_guard<std::mutex> g(mu);
                if (failed) return;
                c = (target.group || want_check) ? nullptr : target.ctx;
            }
            if (c) {  // straight into a staging set
                uint64_t* key;
                int32_t *ref, *pos;
                uint16_t* flag;
                auto t0 = std::chrono::steady_clock::now();
                if (slimm_staging_buffers(c, which, kBatch, &key, &ref, &pos, &flag) < 0) break;  // (waits for the set's last copy)
                auto t1 = std::chrono::steady_clock::now();
                const long n = bam.read_into(key, ref, pos, flag, kBatch);
                auto t2 = std::chrono::steady_clock::now();
                wait_ms += ms(t0, t1);
                decode_ms += ms(t1, t2);
                if (n <= 0) {
                    read_rc = n;
                    return;
                }
                if (marked) {  // (the set's key and flag arrays stay on the host)
                    mark(key, flag, ref, static_cast<uint64_t>(n));
                    if (slimm_push_staged_marked_async(c, which, static_cast<uint64_t>(n)) < 0) break;
                } else {
                    pack(key, flag, static_cast<uint64_t>(n));  // (the set's flag array stays on the host)
                    if (slimm_push_staged_packed_async(c, which, static_cast<uint64_t>(n)) < 0) break;
                }
                which ^= 1u;
                continue;
            }
            Batch b;
            if (want_check) b.check.reset(new uint32_t[kBatch]);
            auto t1 = std::chrono::steady_clock::now();
            const long n = bam.read_into(b.key.get(), b.ref.get(), b.pos.get(), b.flag.get(), kBatch, b.check.get());
            decode_ms += ms(t1, std::chrono::steady_clock::now());
            if (n <= 0) {
                read_rc = n;
                return;
            }
            b.n = static_cast<uint64_t>(n);
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return target.ctx || failed || queued.size() < kMaxQueued; });
            if (failed) return;
            if (target.ctx) {  // attached: everything queued before has been pushed, this batch follows
                if (push(b) < 0) break;
            } else {
                queued.push_back(std::move(b));
            }
        }
        std::lock_guard<std::mutex> g(mu);
        failed = true;
    }
    // pushes what was decoded so far into `t`, hands `t` to the decoder and waits for the end of the file: the threads are
    // joined before this returns, so that `t` may go right after; false on a failed push
    bool drain(Target t) {
        if (raw) {
            raw_pusher = std::thread([this, c = t.ctx] { push_raw(c); });
        } else {
            std::unique_lock<std::mutex> g(mu);
            target = t;
            for (Batch& b : queued)
                if (push(b) < 0) {
                    failed = true;
                    break;
                }
            queued.clear();
            cv.notify_all();
        }
        th.join();
        if (raw_pusher.joinable()) raw_pusher.join();
        return !failed;
    }
    // SLIMM_TRACE=cli: what the threads took (a group: member 0's device decode only)
    void report(bool group) const {
        if (group) {
            if (raw)
                fprintf(stderr, "%sdevice decode on member 0: slimm_push_bam_bytes %.2f ms for %llu records, pusher waited %.2f ms for windows\n",
                        head.c_str(), raw_push_ms, static_cast<unsigned long long>(raw_records), wait_ms);
        } else if (raw) {
            fprintf(stderr, "%sdevice decode: inflate %.2f ms (on its own thread, from the moment the file was open), "
                            "slimm_push_bam_bytes %.2f ms for %llu records, pusher waited %.2f ms for windows; of the windows read in "
                            "place %llu were inflated on the host, %llu on the device\n",
                    head.c_str(), decode_ms, raw_push_ms, static_cast<unsigned long long>(raw_records), wait_ms,
                    static_cast<unsigned long long>(raw_windows_host), static_cast<unsigned long long>(raw_windows_device));
        } else {
            fprintf(stderr, "%sdecode %.2f ms (on its own thread, from the moment the file was open), waiting for staging sets %.2f ms\n",
                    head.c_str(), decode_ms, wait_ms);
        }
    }
};

struct SplitBuffers {   // (page-locked for the life of the group's contexts: they outlive the group)
    struct Map {
        uint8_t* p = nullptr;
        size_t n = 0;
        ~Map() {
            if (p) munmap(p, n);
        }
    };
    std::vector<std::unique_ptr<Map>> maps;
    uint8_t* get(size_t n) {
        void* p = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return nullptr;
        (void)madvise(p, n, MADV_HUGEPAGE);
        maps.emplace_back(new Map{static_cast<uint8_t*>(p), n});
        return static_cast<uint8_t*>(p);
    }
};
// One member's reading of its range of a split file (read_split).  Three buffers: one being read, one being copied, the one
// before it still the library's until the next push
struct SplitMember {
    // set by read_split: the member's context and place, its range [begin, range_end) of the file and where its reads end (the
    // form's slack behind the range -- none behind the file's last --, at most to the file's end), its share of the threads
    const InputForm* form = nullptr;
    slimm_ctx* ctx = nullptr;
    uint32_t index = 0, header_skip = 0;   // (header_skip: member 0's, the header's inflated or decoded bytes)
    bool file_last = false;
    uint64_t begin = 0, range_end = 0, read_end = 0;
    uint64_t begin_bit = 0, end_bit = 0;   // a form cut at bits (announce_bits): the range itself; [begin, range_end) are the bytes that hold it
    int note = -1;   // what the form's range_note said of `begin` (xz: the check kind of the stream around it)
    int fd = -1;
    unsigned threads = 1;
    size_t cap = 0, read_hint = 0;
    uint8_t* buf[3] = {};
    // what it came to
    int rc = SLIMM_OK;
    std::string err;
    uint64_t records = 0;
    double pread_ms = 0, push_ms = 0, last_ms = 0;

    static double ms(std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    }
    // bytes [at, at + n) of the file into dst, by pread on at most `threads` threads (one per MiB); false on a read error
    static bool pread_span(int fd, uint8_t* dst, uint64_t at, size_t n, unsigned threads) {
        const unsigned nt = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(threads, n >> 20)));
        const size_t per = (n + nt - 1) / nt;
        std::atomic<bool> ok{true};
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] {
                const size_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
                if (!pread_all(fd, dst + lo, at + lo, hi - lo)) ok = false;
            });
        for (auto& t : th) t.join();
        return ok;
    }
    // The bytes of the whole BGZF blocks at the front of buf[0, want) (0: none fits).  Blocks of SAM text end a push at
    // `max_inflated` inflated bytes as well (max_inflated_per_push); *read_hint is then set to what is worth reading
    static size_t whole_bgzf_blocks(const uint8_t* buf, size_t want, bool sam, uint64_t max_inflated, size_t* read_hint) {
        size_t n = 0;
        uint64_t inflated = 0;
        while (want - n >= 18) {
            const uint8_t* h = buf + n;
            const size_t bsize = (static_cast<size_t>(h[16]) | (static_cast<size_t>(h[17]) << 8)) + 1u;
            if (h[0] != 0x1f || h[1] != 0x8b || want - n < bsize) break;
            const uint8_t* t = h + bsize - 4;   // (ISIZE)
            const uint64_t isize = !sam || bsize < 28u ? 0u
                                                       : static_cast<uint64_t>(t[0]) | (static_cast<uint64_t>(t[1]) << 8) |
                                                             (static_cast<uint64_t>(t[2]) << 16) | (static_cast<uint64_t>(t[3]) << 24);
            if (n && inflated + isize > max_inflated) {
                *read_hint = n + (n >> 2) + (1u << 16);
                break;
            }
            inflated += isize;
            n += bsize;
        }
        return n;
    }
    // the next push's bytes from `at` on into buffer w: their count -- whole blocks of a BGZF form, else the bytes as they lie
    // there, cut anywhere --, 0 at the end of the reads (or when no block fits), -1 on a read error
    long fill(unsigned w, uint64_t at) {
        const size_t want = static_cast<size_t>(std::min<uint64_t>(std::min(cap, read_hint), read_end - at));
        if (!want) return 0;
        if (!pread_span(fd, buf[w], at, want, threads)) return -1;
        if (form->read != InputForm::Bgzf) return static_cast<long>(want);
        return static_cast<long>(whole_bgzf_blocks(buf[w], want, form->sam, form->sam ? max_inflated_per_push(cap) : ~0ull, &read_hint));
    }
    void failed(int code, const std::string& e) {
        rc = code;
        err = "member " + std::to_string(index) + ": " + e;
    }
    void run(const char* const* names, bool window_pass = false) {
        int r = form->sam ? slimm_set_reference_names(ctx, names) : SLIMM_OK;
        if (r == SLIMM_OK) r = slimm_set_input_mid_file(ctx, index > 0 ? 1 : 0, file_last ? 0 : 1);
        if (r == SLIMM_OK && form->announce_range) r = slimm_set_input_range(ctx, begin, range_end);
        if (r == SLIMM_OK && form->announce_bits) r = form->announce_bits(ctx, begin_bit, end_bit);
        if (r == SLIMM_OK && form->window_pass) r = form->window_pass(ctx, window_pass ? 1 : 0);
        if (r == SLIMM_OK && form->announce_note) r = form->announce_note(ctx, note);
        if (r == SLIMM_OK) r = slimm_set_input_size_hint(ctx, range_end - begin);
        if (r != SLIMM_OK) return failed(r, slimm_last_error(ctx));
        for (auto* b : buf) (void)slimm_pin_host_buffer(ctx, b, cap);   // (pageable memory still works)
        // the next buffer is read while this one is pushed (the one before it is the library's until this push returns)
        read_hint = cap;
        uint64_t pos = begin;
        auto t0 = std::chrono::steady_clock::now();
        long n = fill(0, pos);
        pread_ms += ms(t0);
        for (unsigned w = 0;; w = (w + 1) % 3) {
            if (n < 0) return failed(SLIMM_E_INVALID, "read error");
            if (n == 0 && pos < read_end) return failed(SLIMM_E_INVALID, "a BGZF block does not fit the window");
            const bool last = pos + static_cast<uint64_t>(n) == read_end;
            long next = 0;
            double next_ms = 0;
            std::thread ahead;
            if (!last)
                ahead = std::thread([&, w] {
                    const auto a = std::chrono::steady_clock::now();
                    next = fill((w + 1) % 3, pos + static_cast<uint64_t>(n));
                    next_ms = ms(a);
                });
            uint64_t got = 0;
            t0 = std::chrono::steady_clock::now();
            r = push_window(*form, ctx, buf[w], static_cast<uint64_t>(n), true, pos == begin ? header_skip : 0u, last, &got);
            const double t = ms(t0);
            if (ahead.joinable()) ahead.join();
            pread_ms += next_ms;
            push_ms += t;
            if (last) last_ms = t;
            if (r != SLIMM_OK) return failed(r, slimm_last_error(ctx));
            records += got;
            pos += static_cast<uint64_t>(n);
            n = next;
            if (last) return;
        }
    }
};
// --split-input: every member of a group reads, inflates and decodes its own contiguous byte range of a file -- GROUPED by
// read name or in any order (the stitch then deals the records by key) -- at once, and the library stitches the cuts on the
// devices (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE").  The form's row says how the file is cut and read; member 0
// skips the header's inflated (decoded) bytes; `names`: the header's reference names, for every member's SAM decoder.  The
// reader threads are split over the members, not multiplied (a command gets 16 CPUs).  Returns SLIMM_OK or the code of what
// failed; *why says what.  `planned`: the G + 1 offsets cut_by_byte_range kept, taken when they are for this G (a form without a
// floor, and the cap's re-read with more members: planned here).
int read_split(slimm_group* grp, uint32_t G, const std::string& path, const InputForm& form, const std::vector<std::string>& names,
               uint64_t header_bytes, const std::vector<uint64_t>& planned, size_t window_cap, SplitBuffers& bufs, const char* head, std::string& why) {
    std::vector<uint64_t> off = planned;
    if (off.size() != G + 1u && !plan_ranges(form, path, header_bytes, G, off)) {
        why = std::string("the file's ") + form.planned + " could not be planned into ranges";
        return SLIMM_E_INVALID;
    }
    const uint64_t slack = form.slack ? form.slack() : 0u, file_size = form.announce_bits ? off[G] / 8u : off[G];
    std::vector<const char*> name_ptrs;
    for (const std::string& nm : names) name_ptrs.push_back(nm.c_str());
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) {
        why = "could not open " + path;
        return SLIMM_E_INVALID;
    }
    const unsigned cores = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<SplitMember> m(G);
    std::vector<slimm_ctx*> ctxs(G);
    for (uint32_t i = 0; i < G; ++i) {
        SplitMember& M = m[i];
        M.form = &form, M.fd = fd, M.index = i, M.file_last = i + 1 == G;
        M.ctx = ctxs[i] = slimm_group_context(grp, i);
        M.header_skip = i == 0 ? static_cast<uint32_t>(header_bytes) : 0u;
        M.begin = off[i], M.range_end = off[i + 1];
        if (form.announce_bits) {   // (neighbours share at most one byte)
            M.begin_bit = off[i], M.end_bit = off[i + 1];
            M.begin = off[i] / 8u, M.range_end = (off[i + 1] + 7u) / 8u;
        }
        if (form.range_note && form.range_note(path.c_str(), M.begin, &M.note) != SLIMM_OK) {
            close(fd);
            why = std::string("the file's ") + form.planned + " could not be planned into ranges";
            return SLIMM_E_INVALID;
        }
        M.read_end = std::min<uint64_t>(file_size, M.range_end + (M.file_last ? 0u : slack));
        M.threads = std::max(1u, cores / G);
        M.cap = std::max<size_t>(1u << 20, G <= 2 ? window_cap : window_cap * 2 / G);
        for (auto& b : M.buf)
            if (!(b = bufs.get(M.cap))) {
                close(fd);
                why = "out of host memory for the members' buffers";
                return SLIMM_E_INVALID;
            }
    }
    if (form.window_pass) {   // every member but the last reads its range once for its last 32 768 symbols alone; then they are handed on
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (uint32_t i = 0; i + 1u < G; ++i) th.emplace_back([&m, i, &name_ptrs] { m[i].run(name_ptrs.data(), true); });
        for (auto& t : th) t.join();
        const double pass_ms = SplitMember::ms(t0);
        int rc = SLIMM_OK;
        for (uint32_t i = 0; i + 1u < G && rc == SLIMM_OK; ++i)
            if ((rc = m[i].rc) != SLIMM_OK) why = m[i].err;
        const auto t1 = std::chrono::steady_clock::now();
        if (rc == SLIMM_OK && (rc = form.windows(grp)) != SLIMM_OK) why = slimm_group_last_error(grp);
        if (g_trace)
            fprintf(stderr, "%s%s window pass: %u members read their ranges in %.2f ms, the windows handed on in %.2f ms\n", head, form.name, G - 1u,
                    pass_ms, SplitMember::ms(t1));
        if (rc != SLIMM_OK) {
            close(fd);
            return rc;
        }
        for (SplitMember& M : m) M.records = 0, M.pread_ms = M.push_ms = M.last_ms = 0;
    }
    {
        std::vector<std::thread> th;
        for (SplitMember& M : m) th.emplace_back([&M, &name_ptrs] { M.run(name_ptrs.data()); });
        for (auto& t : th) t.join();
    }
    close(fd);
    for (uint32_t i = 0; i < G && g_trace; ++i)
        fprintf(stderr, "%ssplit member %u: bytes [%llu, %llu) of %llu, %llu records, pread %.2f ms, push %.2f ms, last push (wait) %.2f ms\n", head, i,
                static_cast<unsigned long long>(m[i].begin), static_cast<unsigned long long>(m[i].range_end), static_cast<unsigned long long>(m[G - 1u].range_end),
                static_cast<unsigned long long>(m[i].records), m[i].pread_ms, m[i].push_ms, m[i].last_ms);
    for (uint32_t i = 0; i < G; ++i)
        if (m[i].rc != SLIMM_OK) {
            why = m[i].err;
            return m[i].rc;
        }
    const int rc = slimm_group_stitch_ranges(grp);
    if (rc != SLIMM_OK) why = slimm_group_last_error(grp);
    if (form.end_line && g_trace && rc == SLIMM_OK) form.end_line(head, ctxs.data(), G);   // (the members' counters summed: the whole file's)
    return rc;
}

// One reading of a file up to its context: the file open at its first record, the choices its header and the options make,
// the pump that decodes from the moment the file is open, and the tables slimm_config points into.
struct Reading {
    std::string path;
    Lap watch;
    Trace trace;
    AlignmentFile bam;
    int record_order = SLIMM_ORDER_ANY;
    bool check_words = false;   // the stream is in no particular order: every record carries a second hash of its name
    bool split_input = false;   // --split-input: every member of the group reads its own byte range (read_split): no pump
    std::vector<uint64_t> split_plan;   // ... the G + 1 offsets cut_by_byte_range planned last, for that G (none: read_split plans)
    std::unique_ptr<RecordPump> pump;
    SplitBuffers split_bufs;
    std::vector<std::string> accession;
    std::vector<uint32_t> taxa_id, lineage, tax_id, tax_rank;
    std::vector<const char*> tax_name;
    slimm_config cfg;
};

// write_raw_stat (src/slimm.hpp:883-943) and write_coverage (:846-881) from a context that holds the finished columns and
// coverage arrays.  global_bins: `ctx` is member 0 of a group after the bins exchange -- its arrays are the global ones,
// but its count of non-zero uniq_cov2 bins is that of its own reads: counted here from the global array instead.
Outcome write_raw_and_coverage(Session& S, Reading& F, slimm_ctx* ctx, bool global_bins) {
    const Options& options = S.options;
    const uint32_t R = static_cast<uint32_t>(F.accession.size());
    slimm_stats st;
    slimm_get_stats(ctx, &st);
    std::vector<uint32_t> reads(R), uniq(R), uniq2(R), nbins(R), nz(R), nzu(R), nzu2(R);
    std::vector<uint8_t> valid(R);
    std::vector<float> ab(R), uab(R);
    std::vector<uint32_t> cov, ucov, ucov2;
    if (options.raw_output || options.coverage_output) {
        slimm_ref_columns cols = {reads.data(), uniq.data(), uniq2.data(), nbins.data(), nz.data(),
                                  nzu.data(),   nzu2.data(), valid.data(), ab.data(),    uab.data()};
        CHECK(ctx, slimm_get_ref_columns(ctx, &cols));
        cov.resize(st.total_bins);
        ucov.resize(st.total_bins);
        ucov2.resize(st.total_bins);
        CHECK(ctx, slimm_get_bins(ctx, 0, cov.data()));
        CHECK(ctx, slimm_get_bins(ctx, 1, ucov.data()));
        CHECK(ctx, slimm_get_bins(ctx, 2, ucov2.data()));
        if (global_bins) {  // reference_contig.hpp:84-91 over the global uniq_cov2
            uint64_t off = 0;
            for (uint32_t i = 0; i < R; ++i) {
                uint32_t c = 0;
                for (uint32_t k = 0; k < nbins[i]; ++k) c += ucov2[off + k] != 0u;
                nzu2[i] = c;
                off += nbins[i];
            }
        }
    }
    auto name_of = [&](uint32_t taxid) -> std::string {
        auto it = S.shared->db.taxid_name.find(taxid);
        return it == S.shared->db.taxid_name.end() ? std::string() : it->second.second;
    };
    if (options.raw_output) {  // write_raw_stat :883-943
        S.err() << "Writing features to a file ....................... ";
        std::ofstream o(get_tsv_file_name(options.output_prefix, F.path, "_raw"));
        o << "accesion\ttaxaid\tname\treads_count\tabundance\tuniq1_abundance\tuniq2_abundance\tgenome_length\t"
             "uniq1_reads_count\tuniq2_reads_count\tbins_count\tbins_count(>0)\tuniq1_bins_count(>0)\t"
             "uniq2_bins_count(>0)\tcoverage_depth\tuniq1_coverage_depth\tuniq2_coverage_depth\tcoverage(%)\t"
             "uniq1_coverage(%)\tuniq2_coverage(%)\n";
        uint64_t off = 0;
        for (uint32_t i = 0; i < R; ++i) {
            std::string nm = name_of(F.taxa_id[i]);
            if (nm.empty()) nm = "no_name_found";
            const uint32_t nb = nbins[i];
            o << F.accession[i] << "\t" << F.taxa_id[i] << "\t" << nm << "\t" << reads[i] << "\t" << ab[i] << "\t" << uab[i] << "\t"
              << 0.0f << "\t" << F.bam.ref_lengths()[i] << "\t" << uniq[i] << "\t" << uniq2[i] << "\t" << nb << "\t" << nz[i] << "\t"
              << nzu[i] << "\t" << nzu2[i] << "\t" << depth_of(&cov[off], nb, nz[i]) << "\t" << depth_of(&ucov[off], nb, nzu[i])
              << "\t" << depth_of(&ucov2[off], nb, nzu2[i]) << "\t" << float(nz[i]) / nb << "\t" << float(nzu[i]) / nb << "\t"
              << float(nzu2[i]) / nb << "\n";
            off += nb;
        }
        S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    }
    if (options.coverage_output) {  // write_coverage :846-881
        S.err() << "Writing coverage profiles to a file ....................... ";
        std::ofstream a(get_tsv_file_name(options.output_prefix, F.path, "_coverage"));
        std::ofstream b(get_tsv_file_name(options.output_prefix, F.path, "_uniq_coverage"));
        std::ofstream c(get_tsv_file_name(options.output_prefix, F.path, "_uniq_coverage2"));
        uint64_t off = 0;
        for (uint32_t i = 0; i < R; ++i) {
            const uint32_t nb = nbins[i];
            if (valid[i]) {
                a << F.accession[i];
                b << F.accession[i];
                c << F.accession[i];
                for (int k = 0; k < 8; ++k) {
                    std::string nm = name_of(F.lineage[static_cast<size_t>(i) * 8 + k]);
                    a << "," << nm;
                    b << "," << nm;
                    c << "," << nm;
                }
                for (uint32_t k = 0; k < nb; ++k) {
                    a << "," << cov[off + k];
                    b << "," << ucov[off + k];
                    c << "," << ucov2[off + k];
                }
                a << "\n";
                b << "\n";
                c << "\n";
            }
            off += nb;
        }
        S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    }

    return Outcome::Done;
}

// average read length from a sample of 100k records with a sequence (src/misc.hpp:509-522); 0: no record has one
uint32_t average_read_length(AlignmentFile& bam) {
    RecordBatch b;
    uint32_t count = 0, total = 0;
    while (count < 100000) {
        b.clear();
        long n = bam.read_batch(b, 4096);
        if (n <= 0) break;
        for (size_t i = 0; i < b.size() && count < 100000; ++i) {
            if (b.l_seq[i] == 0) continue;
            total += b.l_seq[i];
            ++count;
        }
    }
    return count ? total / count : 0;
}

// Opens the file and sets a reading of it up (src/slimm.hpp:395-445).  any_order: the second reading of a file that asked
// for the any-order path.  nullptr when the file ends here: `end` says how (Done: skipped, src/misc.hpp:500-504).
std::unique_ptr<Reading> set_up(Session& S, const std::string& path, bool any_order, Outcome& end) {
    Options& options = S.options;
    std::unique_ptr<Reading> F(new Reading);
    F->path = path;
    F->trace.head = S.log->head;
    AlignmentFile& bam = F->bam;
    bam.set_trace_head(S.log->head);
    if (options.filtered()) bam.set_filter(options.filter);
    end = Outcome::Done;
    if (!bam.open(path)) {  // src/misc.hpp:500-504: message, skip the file
        S.err() << bam.error() << "\n";
        return nullptr;
    }
    const uint32_t avg_read_length = average_read_length(bam);
    if (avg_read_length == 0) {
        S.err() << "[ERROR] no record with a sequence in " << path << " (the reference divides by zero here)\n";
        end = Outcome::Failed;
        return nullptr;
    }
    if (options.bin_width == 0) options.bin_width = avg_read_length;  // :412-413, persists across files
    F->trace.mark("open + read-length sample");
    if (!reopen(bam, path, S.err())) return nullptr;
    // only a header that promises name grouping is trusted; anything else is sorted on the device
    F->record_order = any_order ? SLIMM_ORDER_ANY
                      : options.order >= 0
                          ? options.order
                          : ((bam.sort_order() == SortOrder::QueryName || bam.sort_order() == SortOrder::QueryGrouped)
                                 ? SLIMM_ORDER_GROUPED
                                 : SLIMM_ORDER_ANY);
    // (grouped streams are exact already: the reader compares the names of adjacent records)
    F->check_words = F->record_order == SLIMM_ORDER_ANY;
    // decoding starts now; the records are claimed further down, when the context exists (one context: the device decodes)
    // (a group takes a file through member 0's device decoders and deals the records device to device afterwards --
    // slimm_group_get_profiles: a GROUPED file in stretches cut at qName runs, any other order by key; what the pump does
    // not push raw -- --host-decode, pipes ... -- the host reader deals)
    const bool may_split = options.split_input && options.devices.size() > 1 && !options.host_decode && !options.verify_grouping && !options.packed_records;
    F->split_input = may_split && cut_by_byte_range(bam, path, static_cast<uint32_t>(options.devices.size()), true, &F->split_plan);
    // (a form that is not cut whenever it is asked: a gzip file of one dynamic block, or one whose members would get less bytes
    // than its floor; a zstd file of one frame, or one whose members would get less
    // bytes than its floor; an xz file the host reader takes, or one whose members would get fewer blocks than its floor; or
    // the host decoders were asked for)
    const InputForm& form = form_of(bam);
    if (g_trace && !any_order && !F->split_input && options.split_input && options.devices.size() > 1 && (!form.plan || form.split_floor))
        fprintf(stderr, "%s--split-input: %s %s stream is not cut by byte range; member 0 reads %s\n", S.trace_head(), form.article, form.name, path.c_str());
    if (!F->split_input) {
        // (a regular file that its form gives to the host reader -- an xz file of few blocks --: the pump's host path)
        Options pump_options = options;
        const bool device_asked = !options.host_decode && !options.verify_grouping && !options.packed_records;
        if (form.by_host && device_asked && has_raw_windows(bam) && form.by_host(path, S.trace_head())) pump_options.host_decode = true;
        F->pump.reset(new RecordPump(bam, F->check_words, true, pump_options, S.log->head));
    }

    S.err() << "Intializing coverages for all reference genome ... ";
    const uint32_t R = static_cast<uint32_t>(bam.ref_names().size());
    F->accession.resize(R);
    F->taxa_id.assign(R, 0);
    F->lineage.assign(static_cast<size_t>(R) * 8, 0);
    SlimmDatabase& db = S.shared->db;
    std::vector<uint32_t> unknown;
    {   // :430-445
        std::shared_lock<std::shared_mutex> g(S.shared->db_mu);
        for (uint32_t i = 0; i < R; ++i) {
            F->accession[i] = get_accession_id(bam.ref_names()[i]);
            auto it = db.ac_taxid.find(F->accession[i]);
            if (it != db.ac_taxid.end()) {
                F->taxa_id[i] = it->second.empty() ? 0 : it->second[0];
                for (size_t k = 0; k < 8 && k < it->second.size(); ++k) F->lineage[static_cast<size_t>(i) * 8 + k] = it->second[k];
            } else {
                unknown.push_back(i);
            }
        }
    }
    if (!unknown.empty()) {
        // Q13: an unknown accession gets a zero lineage in the database.  Whoever looks it up later -- this file, for a name its
        // header holds twice, or another one -- reads the zeros it would have got for a missing entry, so it does not matter who
        // inserts first; the writers only may not meet the readers above
        std::unique_lock<std::shared_mutex> g(S.shared->db_mu);
        for (uint32_t i : unknown) db.ac_taxid.emplace(F->accession[i], std::vector<uint32_t>(8, 0));
    }
    F->tax_id.reserve(db.taxid_name.size());
    for (auto& kv : db.taxid_name) {
        F->tax_id.push_back(kv.first);
        F->tax_rank.push_back(kv.second.first);
        F->tax_name.push_back(kv.second.second.c_str());
    }
    slimm_config& cfg = F->cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.n_refs = R;
    cfg.ref_len = bam.ref_lengths().data();
    cfg.lineage = F->lineage.data();
    cfg.bin_width = options.bin_width;
    cfg.avg_read_len = avg_read_length;
    cfg.min_reads = options.min_reads;
    cfg.cov_cut_off = options.cov_cut_off;
    cfg.abundance_cut_off = options.abundance_cut_off;
    cfg.rank = options.rank.c_str();
    cfg.n_taxa = static_cast<uint32_t>(F->tax_id.size());
    cfg.tax_id = F->tax_id.data();
    cfg.tax_rank = F->tax_rank.data();
    cfg.tax_name = F->tax_name.data();
    cfg.device = options.device;
    cfg.record_order = F->record_order;
    return F;
}

// What a push that found more records than one context takes leads to (the --split-input reading decides in run_group):
// a group reading through member 0 -- HostDecode, the host reader deals them; one context of a file whose form is cut
// (kForms), grouped or in any order -- MoreMembers, a group on the device reads the file by byte range; any other one context -- Fail.
enum class OnCap { Fail, HostDecode, MoreMembers };

// The file's records through F.pump into `t`: Done, or Failed with the reason printed.  A record longer than the device
// decoder's carry (16 MiB) resets `t`, reopens the file and sends it through the host decoder after all; more records than
// one context takes go by `on_cap`.
Outcome push_file(Session& S, Reading& F, Target t, OnCap on_cap) {
    RecordPump& pump = *F.pump;
    bool ok = pump.drain(t);
    long read_rc = pump.read_rc;
    if (F.trace.on) pump.report(t.group != nullptr);
    if (!t.group) F.trace.mark("rest of read + decode + push");   // (one context: the host decoder's pass is not in the mark)
    const PushError why = ok || !pump.raw || read_rc < 0 ? PushError::Other : classify(slimm_last_error(t.ctx));
    if (why == PushError::RecordCap && on_cap == OnCap::MoreMembers) return Outcome::MoreMembers;
    if (why == PushError::HostDecode || (why == PushError::RecordCap && on_cap == OnCap::HostDecode)) {
        S.err() << "(" << slimm_last_error(t.ctx) << ": decoding on the host) ";
        if (t.reset() != SLIMM_OK) {
            S.err() << "slimm: " << (t.group ? "" : "slimm_reset(ctx): ") << t.error() << "\n";
            return Outcome::Failed;
        }
        if (!reopen(F.bam, F.path, S.err())) return Outcome::Failed;
        RecordPump again(F.bam, F.check_words, false, S.options, S.log->head);
        ok = again.drain(t);
        read_rc = again.read_rc;
    }
    if (t.group) F.trace.mark("rest of read + decode + push");
    if (!ok) {   // (a pump that fed the device decoders: their context's message, after the host decoder's pass too)
        S.err() << (t.group ? "" : "slimm: ") << "pushing records: " << (pump.raw ? slimm_last_error(t.ctx) : t.error()) << "\n";
        return Outcome::Failed;
    }
    if (read_rc < 0) {
        S.err() << F.bam.error() << "\n";
        return Outcome::Failed;
    }
    return Outcome::Done;
}

// Q17: one line per file whose propagated read counts depend on the order of the walk, or could not be shown not to
// (slimm_get_propagation_order on the context that propagated).  The profile is written either way.
void warn_propagation_order(slimm_ctx* ctx, const std::string& path, int walk, std::ostream& err) {
    int verdict = SLIMM_PROPAGATION_INDEPENDENT;
    uint32_t n = 0;
    if (slimm_get_propagation_order(ctx, &verdict, nullptr, 0, &n) != SLIMM_OK || verdict == SLIMM_PROPAGATION_INDEPENDENT) return;
    std::vector<uint32_t> taxa(std::max<uint32_t>(n, 1u));
    if (slimm_get_propagation_order(ctx, &verdict, taxa.data(), n, &n) != SLIMM_OK) return;
    const uint32_t shown = std::min<uint32_t>(n, 12u);
    std::ostringstream line;
    line << "[WARNING] " << get_file_name(path) << ": the propagated read counts "
         << (verdict == SLIMM_PROPAGATION_DEPENDENT ? "depend on the order in which the directly counted taxa are walked"
                                                    : "could not be shown independent of the order in which the directly counted taxa are walked")
         << " (lineage holes; the " << (walk == SLIMM_WALK_REVERSED ? "reversed" : "default") << " walk was taken, see --propagation-walk); taxid"
         << (n == 1 ? "" : "s") << " involved:";
    for (uint32_t k = 0; k < shown; ++k) line << ' ' << taxa[k];
    if (n > shown) line << " and " << n - shown << " more";
    err << line.str() << std::endl;
}

// The record filter's line of a file: what the device decoders judged (member 0 of a group: all members) and what the host
// reader judged of the records it decoded itself -- a record goes through one of the two
void log_filter_stats(Session& S, Reading& F, slimm_ctx* ctx) {
    uint64_t st[SLIMM_RF_N_STATS] = {};
    (void)slimm_get_record_filter_stats(ctx, st);
    for (int k = 0; k < SLIMM_RF_N_STATS; ++k) st[k] += F.bam.filter_stats()[k];
    S.err() << "  " << filter_stats_line(st) << std::endl;
}

// ---- several GPUs, one process (--devices), or members of a group on ONE device for a file of more records than one
// context takes (for_cap): the group deals the records to its members by read and runs the phases with the two RCCL
// exchanges in between (slimm_amd/csrc/group.hip); the profile comes from member 0
Outcome run_group(Session& S, Reading& F, const std::vector<int>& devs, bool split, bool for_cap) {
    Options& options = S.options;
    slimm_group* created = nullptr;
    {   // (a failed slimm_group_create leaves its message in one string of the process: one at a time, for the slots of
        // --file-per-device, whose files may each meet the record cap)
        static std::mutex create_mu;
        std::lock_guard<std::mutex> g(create_mu);
        if (slimm_group_create(&F.cfg, devs.data(), static_cast<uint32_t>(devs.size()), &created) != SLIMM_OK) {
            S.err() << "slimm: " << slimm_group_last_error(nullptr) << "\n";
            return Outcome::Failed;
        }
    }
    const GroupPtr grp(created, slimm_group_destroy);
    const bool want_arrays = options.raw_output || options.coverage_output;
    // -ro / -co read the coverage arrays (src/slimm.hpp:846-943): the members then exchange the integer bins themselves
    // (ncclAllReduce over [cov | uniq_cov], and over uniq_cov2 behind phase B) instead of their summaries
    if (want_arrays) (void)slimm_group_set_exchange(grp.get(), SLIMM_EXCHANGE_BINS);
    for (uint32_t i = 0; i < devs.size(); ++i) {
        (void)slimm_set_cutoff_cache(slimm_group_context(grp.get(), i), S.cc_cache, S.ucc_cache);
        (void)slimm_keep_bins(slimm_group_context(grp.get(), i), want_arrays ? 1 : 0);
    }
    slimm_ctx* c0 = slimm_group_context(grp.get(), 0);
    (void)slimm_set_propagation_walk(c0, options.propagation_walk);   // (member 0 propagates)
    if (options.filtered() && slimm_group_set_record_filter(grp.get(), &options.filter) != SLIMM_OK) {
        S.err() << "slimm: " << slimm_group_last_error(grp.get()) << "\n";
        return Outcome::Failed;
    }
    F.trace.mark("lineage table + slimm_group_create");
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    S.err() << "Analysing alignments on " << devs.size() << " devices ("
              << (slimm_group_uses_rccl(grp.get()) ? "RCCL" : "copy") << " collectives) ... ";
    bool split_read = false;
    if (split) {   // every member its own byte range (read_split); what fails there goes through member 0 after all
        std::string why;
        const InputForm& split_form = form_of(F.bam);
        const int src = read_split(grp.get(), static_cast<uint32_t>(devs.size()), F.path, split_form, F.bam.ref_names(), planned_header_bytes(split_form, F.bam),
                                   F.split_plan, RecordPump::raw_cap(), F.split_bufs, S.trace_head(), why);
        F.trace.mark("split: read + decode + stitch");
        if (src == SLIMM_E_REGROUP) return Outcome::ReadAgainAnyOrder;
        if (src != SLIMM_OK && for_cap && classify(why.c_str()) == PushError::RecordCap) return Outcome::MoreMembers;
        if (src != SLIMM_OK) {
            S.err() << "(split input: " << why << "; reading the file through member 0) ";
            if (slimm_group_reset(grp.get()) != SLIMM_OK) {
                S.err() << "slimm: " << slimm_group_last_error(grp.get()) << "\n";
                return Outcome::Failed;
            }
            if (!reopen(F.bam, F.path, S.err())) return Outcome::Failed;
        }
        split_read = src == SLIMM_OK;
    }
    if (!split_read) {   // member 0 reads the whole file
        if (!F.pump) F.pump.reset(new RecordPump(F.bam, F.check_words, true, options, S.log->head));
        if (F.pump->raw) set_size_hint(c0, F.path);   // (what member 0 sizes its window buffers by)
        const Outcome pushed = push_file(S, F, Target{c0, grp.get()}, OnCap::HostDecode);
        if (pushed != Outcome::Done) return pushed;
    }
    if (F.record_order == SLIMM_ORDER_GROUPED && F.bam.q18_regroup_needed()) return Outcome::ReadAgainAnyOrder;
    const int grc = slimm_group_get_profiles(grp.get(), get_tsv_file_name(options.output_prefix, F.path, "_profile").c_str());
    if (grc == SLIMM_E_REGROUP) return Outcome::ReadAgainAnyOrder;   // (member 0's decoders counted a run of shortened names only: Q18)
    if (grc < 0) {
        S.err() << "slimm: " << slimm_group_last_error(grp.get()) << "\n";
        return Outcome::Failed;
    }
    F.trace.mark("phases + exchanges + profile");
    if (F.trace.on) trace_memory(c0, S.trace_head());
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    if (options.filtered()) log_filter_stats(S, F, c0);
    slimm_stats st;
    slimm_get_stats(c0, &st);
    S.total_hits += st.hits_count;
    if (grc == SLIMM_E_NO_HITS) {
        S.err() << "[WARNING] No mapped reads found in BAM file!" << std::endl;
        return Outcome::Done;
    }
    warn_propagation_order(c0, F.path, options.propagation_walk, S.err());
    if (options.min_reads == 0) options.min_reads = st.min_reads;
    if (options.verbose) {
        S.err() << "  " << st.hits_count << " records processed." << std::endl;
        S.err() << "    " << st.matches_count << " matching reads" << std::endl;
        S.err() << "    " << st.uniq_matches_count << " uniquily matching reads" << std::endl;
        S.err() << "  references with reads = " << st.reference_count << std::endl;
        S.err() << "  " << st.n_valid << " passed the threshould coverage.\n";
        S.err() << "  uniquily matching reads increased from " << st.uniq_matches_count << " to " << st.uniq_matches_count2 << "\n";
        S.err() << std::setw(4) << st.profile_count << std::setw(15) << (options.rank) << " (" << st.profile_failed
                  << " bellow cutoff i.e. " << options.abundance_cut_off << ")\n";
    }
    if (want_arrays && write_raw_and_coverage(S, F, c0, true) != Outcome::Done) return Outcome::Failed;
    S.err() << "[Done!] File took " << F.watch.elapsed() << " secs to process.\n";
    (void)slimm_get_cutoff_cache(c0, &S.cc_cache, &S.ucc_cache);
    return Outcome::Done;
}

Outcome run_context(Session& S, Reading& F) {
    Options& options = S.options;
    slimm_ctx* created = nullptr;
    if (slimm_create(&F.cfg, &created) != SLIMM_OK) {
        S.err() << "slimm: " << slimm_last_error(nullptr) << "\n";
        return Outcome::Failed;
    }
    CtxPtr owned(created, slimm_destroy);
    slimm_ctx* ctx = owned.get();
    CHECK(ctx, slimm_set_cutoff_cache(ctx, S.cc_cache, S.ucc_cache));
    CHECK(ctx, slimm_set_propagation_walk(ctx, options.propagation_walk));
    if (options.filtered()) CHECK(ctx, slimm_set_record_filter(ctx, &options.filter));
    set_size_hint(ctx, F.path);
    slimm_keep_bins(ctx, (options.raw_output || options.coverage_output) ? 1 : 0);  // (only -ro / -co read the arrays back)
    F.trace.mark("lineage table + slimm_create");
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;

    S.err() << "Analysing alignments, reads and references ....... ";
    // (gzip, zstd and xz SAM: whether the file can be cut is asked only once the cap is met -- the plan reads the file; the floor is
    // not consulted here.  A zstd file of one frame, an xz file of one block behind the header's or one that the host reader
    // took -- fewer than xz_device_blocks() blocks -- cannot be cut and ends at the cap, as it did)
    const InputForm& form = form_of(F.bam);
    const Outcome pushed = push_file(S, F, Target{ctx}, F.bam.regular_file() && form.plan ? OnCap::MoreMembers : OnCap::Fail);
    if (pushed == Outcome::MoreMembers && !cut_by_byte_range(F.bam, F.path, 2u, false, &F.split_plan)) {
        S.err() << "slimm: pushing records: " << slimm_last_error(ctx) << "\n";
        return Outcome::Failed;
    }
    if (pushed == Outcome::MoreMembers) {
        // more records than one context takes: contexts of a group on this one device, each its own byte range of the
        // file (read_split) -- twice as many until each range fits
        S.err() << "(" << slimm_last_error(ctx) << ": reading the file by byte range into several contexts of device " << options.device
                  << ") ";
        const uint64_t records = F.pump->raw_records;
        owned.reset();
        F.pump.reset();
        const uint64_t cap = slimm_record_cap();
        uint32_t G = std::max<uint32_t>(2u, static_cast<uint32_t>(std::min<uint64_t>(64u, 2u * (records + cap - 1) / cap)));
        for (; G <= 128u; G *= 2u) {
            if (!reopen(F.bam, F.path, S.err())) return Outcome::Failed;
            const Outcome r = run_group(S, F, std::vector<int>(G, options.device), true, true);
            if (r != Outcome::MoreMembers) return r;
        }
        S.err() << "slimm: more records than " << G / 2 << " contexts take\n";
        return Outcome::Failed;
    }
    if (pushed != Outcome::Done) return pushed;
    if (F.record_order == SLIMM_ORDER_GROUPED && options.verify_grouping) {
        // the header (or --query-grouped) promises that the records of a read name are adjacent; nothing checks the promise
        // unless asked: a name that comes back later would be counted as two reads (include/slimm_hip.h, slimm_check_grouping)
        uint64_t split = 0;
        CHECK(ctx, slimm_check_grouping(ctx, &split));
        if (split)
            S.err() << "\n[WARNING] " << split << " read name run(s) repeat a name seen earlier in " << get_file_name(F.path)
                      << ": the file is NOT grouped by read name although it is declared so; run with --any-order\n";
    }
    // (the device decoders count inside the library: SLIMM_E_REGROUP; the host decoder counts in the reader)
    if (F.record_order == SLIMM_ORDER_GROUPED && F.bam.q18_regroup_needed()) return Outcome::ReadAgainAnyOrder;
    const int arc = slimm_analyze_alignments(ctx);
    if (arc == SLIMM_E_REGROUP) return Outcome::ReadAgainAnyOrder;
    if (arc < 0) {
        S.err() << "slimm: slimm_analyze_alignments(ctx): " << slimm_last_error(ctx) << "\n";
        return Outcome::Failed;
    }
    const int rc = slimm_finish_coverage(ctx);
    if (rc < 0) {
        S.err() << "slimm: " << slimm_last_error(ctx) << "\n";
        return Outcome::Failed;
    }
    F.trace.mark("analyze_alignments + finish_coverage");
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    if (options.filtered()) log_filter_stats(S, F, ctx);
    slimm_stats st;
    slimm_get_stats(ctx, &st);
    S.total_hits += st.hits_count;
    if (rc == SLIMM_E_NO_HITS) {
        S.err() << "[WARNING] No mapped reads found in BAM file!" << std::endl;
        return Outcome::Done;
    }
    if (options.min_reads == 0) options.min_reads = st.min_reads;  // :458-459, persists across files
    if (options.verbose) {                                         // print_matches_stat :621-630
        S.err() << "  " << st.hits_count << " records processed." << std::endl;
        S.err() << "    " << st.matches_count << " matching reads" << std::endl;
        S.err() << "    " << st.uniq_matches_count << " uniquily matching reads" << std::endl;
        S.err() << "  references with reads = " << st.reference_count << std::endl;
        S.err() << "  expected bins coverage = " << st.expected_coverage << std::endl;
        S.err() << "  bins coverage cut-off = " << st.coverage_cut_off << " (" << options.cov_cut_off << " quantile)\n";
        S.err() << "  uniq bins coverage cut-off = " << st.uniq_coverage_cut_off << " (" << options.cov_cut_off << " quantile)\n\n";
    }

    S.err() << "Filtering unlikely sequences ..................... ";
    CHECK(ctx, slimm_filter_alignments(ctx));
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    slimm_get_stats(ctx, &st);
    if (options.verbose) {  // print_filter_stat :613-619
        S.err() << "  " << st.n_valid << " passed the threshould coverage.\n";
        S.err() << "  " << st.failed_by_cov << " ref's couldn't pass the coverage threshould.\n";
        S.err() << "  " << st.failed_by_uniq_cov << " ref's couldn't pass the uniq coverage threshould.\n";
        S.err() << "  uniquily matching reads increased from " << st.uniq_matches_count << " to " << st.uniq_matches_count2 << "\n\n";
    }

    if ((options.raw_output || options.coverage_output) && write_raw_and_coverage(S, F, ctx, false) != Outcome::Done) return Outcome::Failed;
    S.err() << "Assigning reads to Least Common Ancestor (LCA) ... ";
    CHECK(ctx, slimm_get_reads_lca_count(ctx));
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    warn_propagation_order(ctx, F.path, options.propagation_walk, S.err());

    S.err() << "Writing taxnomic profile(s) ...................... ";
    CHECK(ctx, slimm_write_abundance_file(ctx, get_tsv_file_name(options.output_prefix, F.path, "_profile").c_str()));
    if (options.verbose) {
        slimm_get_stats(ctx, &st);
        S.err() << "\n" << std::setw(4) << st.profile_count << std::setw(15) << (options.rank) << " (" << st.profile_failed
                  << " bellow cutoff i.e. " << options.abundance_cut_off << ")";
        S.err() << "\n.................................................. ";
    }
    S.err() << "[" << F.watch.lap() << " secs]" << std::endl;
    F.trace.mark("filter + LCA + outputs");
    if (F.trace.on) trace_memory(ctx, S.trace_head());
    S.err() << "[Done!] File took " << F.watch.elapsed() << " secs to process.\n";
    CHECK(ctx, slimm_get_cutoff_cache(ctx, &S.cc_cache, &S.ucc_cache));
    owned.reset();
    F.trace.mark("slimm_destroy");
    return Outcome::Done;
}

// slimm::get_profiles() for one file (src/slimm.hpp:395-496)
bool get_profiles(Session& S, size_t file_index) {
    const std::string& path = S.shared->input_paths[file_index];
    S.err() << "\nReading " << file_index + 1 << " of " << S.shared->input_paths.size() << " files ... (" << get_file_name(path) << ")\n"
              << "=================================================================\n";
    auto read = [&](bool any_order) {   // one reading of the file, through a group (--devices) or one context
        Outcome end;
        std::unique_ptr<Reading> F = set_up(S, path, any_order, end);
        if (!F) return end;
        return S.options.devices.size() > 1 ? run_group(S, *F, S.options.devices, F->split_input, false) : run_context(S, *F);
    };
    Outcome r = read(false);
    if (r == Outcome::ReadAgainAnyOrder) {
        // Q18 on a file grouped by QNAME (include/slimm_hip.h, "Q18 ON A GROUPED STREAM"): a read named `r.1` without a mate
        // flag is the reference's read of the first-in-pair records of `r`, wherever those lie in the file
        // (src/slimm.hpp:204-211).  The readers count the runs of such shortened names that stand apart from their
        // namesakes; a file that has one is read again, in any order (a fresh context of the same process: the HIP runtime
        // and the page cache are warm).  The any-order path never asks for it.
        S.err() << "\n(read names ending in .1 / .2 without a mate flag, apart from the flagged records of the shortened name: "
                     "reading " << get_file_name(path) << " again as a file in no particular order)\n";
        r = read(true);
    }
    return r == Outcome::Done;
}

// --file-per-device: the files of S.shared->input_paths, in that order, through the slots of S.options.slots; false when a
// file failed (the sequential run's status 1).  Two steps.  (1) The files are read in turn in slot 0 -- S itself, carrying
// its values from file to file exactly as main()'s loop does -- until those values are settled (Session::settled): up to
// there a file's result depends on the files before it.  (2) The rest is handed, in list order, to whichever slot is free;
// a slot is a thread with a copy of the settled values and its own device, and reads a file as --device N does -- the device
// decoders and their fallbacks, the any-order re-read, the re-read by byte range into several contexts of ITS device at the
// record cap.  No group spans slots.  If the values never settle -- a directory of files without mapped reads -- step 1 takes
// every file.  Every output file is byte for byte the sequential run's.
// A file's stderr lines are collected (FileLog) and printed as one block, the blocks in list order: a finished block waits
// for those before it.  The first failing file in list order has the last block printed; once a failure is known no new file
// starts, the running ones finish (so outputs of files behind the failing one may exist).
bool run_file_per_device(Session& S) {
    const std::vector<std::string>& paths = S.shared->input_paths;
    const size_t n = paths.size(), n_slots = S.options.slots.size();
    struct Board {
        std::mutex mu;
        std::vector<std::string> block;   // of the finished files not printed yet
        std::vector<int> state;           // 0: not finished, 1: done, 2: failed
        size_t printed = 0;               // blocks [0, printed) are out
        bool closed = false;              // ... the last of them a failed file's: nothing follows it
        size_t next = 0;                  // the next file to hand out
        bool failure = false;             // a file failed: no new one starts
        uint32_t hits = 0;                // (total_hits: a sum modulo 2^32, whatever the order)
    } board;
    board.block.resize(n);
    board.state.assign(n, 0);
    auto one_file = [&](Session& mine, size_t k, size_t slot) {
        FileLog log;
        log.collect = true;
        log.head = "[trace] file " + std::to_string(k + 1) + ": ";
        FileLog* const before = mine.log;
        mine.log = &log;
        if (g_trace)
            fprintf(stderr, "[trace] file-per-device: file %zu (%s) in slot %zu on device %d\n", k + 1, get_file_name(paths[k]).c_str(), slot,
                    mine.options.device);
        Trace trace;
        trace.head = log.head;
        const bool ok = get_profiles(mine, k);
        trace.mark("get_profiles + its buffers released");
        mine.log = before;
        std::lock_guard<std::mutex> g(board.mu);
        board.block[k] = log.block.str();
        board.state[k] = ok ? 1 : 2;
        if (!ok) board.failure = true;
        for (; !board.closed && board.printed < n && board.state[board.printed]; ++board.printed) {
            // (one call: stderr is not buffered, so the block goes out whole, between the [trace] lines of other threads)
            fwrite(board.block[board.printed].data(), 1, board.block[board.printed].size(), stderr);
            std::string().swap(board.block[board.printed]);
            board.closed = board.state[board.printed] == 2;
        }
        return ok;
    };
    size_t in_turn = 0;
    for (; in_turn < n && !S.settled(); ++in_turn)
        if (!one_file(S, in_turn, 0)) return false;
    if (g_trace)
        fprintf(stderr, "[trace] file-per-device: %zu of %zu files read in turn before the carried values settled; %zu handed to %zu slots\n",
                in_turn, n, n - in_turn, n_slots);
    board.next = in_turn;
    std::vector<std::thread> slots;
    for (size_t j = 0; j < std::min(n_slots, n - in_turn); ++j)
        slots.emplace_back([&, j] {
            Session mine = S;   // (its own copy of the options: the re-read at the record cap asks them for the device)
            mine.options.device = S.options.slots[j];
            mine.total_hits = 0;
            for (;;) {
                size_t k;
                {
                    std::lock_guard<std::mutex> g(board.mu);
                    if (board.failure || board.next >= n) break;
                    k = board.next++;
                }
                if (!one_file(mine, k, j)) break;
                if (mine.options.bin_width != S.options.bin_width || mine.options.min_reads != S.options.min_reads ||
                    mine.cc_cache != S.cc_cache || mine.ucc_cache != S.ucc_cache) {   // (what settled() rules out)
                    std::lock_guard<std::mutex> g(board.mu);
                    std::cerr << "slimm: " << get_file_name(paths[k]) << " changed a value carried from file to file after those had settled\n";
                    board.failure = true;
                    break;
                }
            }
            std::lock_guard<std::mutex> g(board.mu);
            board.hits += mine.total_hits;
        });
    for (std::thread& t : slots) t.join();
    S.total_hits += board.hits;
    return !board.failure;
}

}  // namespace

int main(int argc, char** argv) {
    {   // SLIMM_TRACE=cli | all | 1 (a comma list; host / push are the library's: slimm_amd/csrc/force.h)
        const char* e = getenv("SLIMM_TRACE");
        for (const char* p = e; p && *p;) {
            const char* end = strchr(p, ',');
            const size_t len = end ? static_cast<size_t>(end - p) : strlen(p);
            if ((len == 3 && (!memcmp(p, "cli", 3) || !memcmp(p, "all", 3))) || (len == 1 && *p == '1')) g_trace = true;
            if (!end) break;
            p = end + 1;
        }
        AlignmentFile::settings().trace = g_trace;
    }
    if (g_trace) {
        struct timespec now;
        clock_gettime(CLOCK_REALTIME, &now);
        fprintf(stderr, "[trace] main() entered at %.6f (epoch seconds)\n", now.tv_sec + now.tv_nsec * 1e-9);
    }
    Shared shared;
    FileLog direct;
    Session S;
    S.shared = &shared;
    S.log = &direct;
    int pr = parse(argc, argv, S.options);
    if (pr == 2) return 0;
    if (pr != 0) return 1;
    if (S.options.window_mb && !S.options.dump_records) RecordPump::raw_cap_setting() = static_cast<size_t>(S.options.window_mb) << 20;
    if (S.options.dump_records) return dump_records(S.options);
    // the HIP runtime starts (0.1 - 0.3 s) while the database is loaded and the first file opened and sampled
    struct WarmUp {
        std::thread t;
        ~WarmUp() {
            if (t.joinable()) t.join();
        }
    } warm_up{std::thread([devices = S.options.file_per_device ? S.options.slots : S.options.devices.size() > 1 ? S.options.devices : std::vector<int>{S.options.device}] { lazy::load(devices); })};
    Lap watch;
    // slimm::slimm(): collect_bam_files + load_slimm_database (src/slimm.hpp:96-101, 306-326)
    if (S.options.is_directory) {
        shared.input_paths = get_bam_files_in_directory(S.options.input_path);
        if (S.options.verbose)
            std::cerr << shared.input_paths.size() << " SAM/BAM Files found under the directory: " << S.options.input_path << "!\n";
    } else if (access(S.options.input_path.c_str(), 0) == 0) {
        shared.input_paths.push_back(S.options.input_path);
    } else {
        std::cerr << S.options.input_path << " is not a file use -d option for a directory.\n";
        return 1;
    }
    std::string err;
    Trace trace;
    if (!load_slimm_database(S.options.database_path, shared.db, err)) {
        std::cerr << "slimm: " << err << "\n";
        return 1;
    }
    trace.mark("load .sldb");
    auto closing_lines = [&] {
    std::cerr << "\n*****************************************************************\n";
        std::cerr << S.total_hits << " SAM/BAM alignment records are proccessed.\n";
        std::cerr << "Taxonomic profiles are written to: \n   " << get_directory(S.options.output_prefix) << "\n";
        std::cerr << "Total time elapsed: " << watch.elapsed() << " secs\n";
        if (trace.on) {
            // since exec(): /proc/self/stat field 22 is the start time in clock ticks since boot
            double up = 0;
            if (FILE* f = fopen("/proc/uptime", "r")) {
                if (fscanf(f, "%lf", &up) != 1) up = 0;
                fclose(f);
            }
            unsigned long long start_ticks = 0;
            if (FILE* f = fopen("/proc/self/stat", "r")) {
                char buf[2048];
                if (fgets(buf, sizeof buf, f)) {
                    const char* p = strrchr(buf, ')');
                    int field = 2;
                    for (p = p ? p + 1 : buf; *p && field < 22; ++p)
                        if (*p == ' ') ++field;
                    start_ticks = strtoull(p, nullptr, 10);
                }
                fclose(f);
            }
            const double since_exec = up - static_cast<double>(start_ticks) / sysconf(_SC_CLK_TCK);
            fprintf(stderr, "[trace] main() reached its end %.0f ms after exec (10 ms resolution)\n", since_exec * 1e3);
            struct timespec now;
            clock_gettime(CLOCK_REALTIME, &now);
            fprintf(stderr, "[trace] leaving at %.6f (epoch seconds)\n", now.tv_sec + now.tv_nsec * 1e-9);
        }
        // (Every output file is written and closed.  Leaving through _exit here, without the teardown in this process, measured
        // SLOWER end to end since the window buffers are page-locked: the kernel driver then takes the process's queues, pinned
        // pages and device memory back on its own -- 0.20 - 0.23 s from _exit to the parent's wait() returning against 0.07 s of
        // orderly teardown + 0.09 s; round 4.  Round 6: _exit behind our own release of everything -- only the runtime's
        // atexit teardown skipped -- is inside the run-to-run noise of 0.64 - 0.84 s, profiles/round6/05_exit_experiment.txt.)
        std::cerr.flush();
        fflush(nullptr);
    };
    if (S.options.file_per_device) {
        // (up to 64 decode threads a file by default: shared among the files open at once; --decode-threads N is per file)
        const unsigned at_once = static_cast<unsigned>(std::max<size_t>(1, std::min(S.options.slots.size(), shared.input_paths.size())));
        if (AlignmentFile::settings().threads == 0) AlignmentFile::settings().threads = std::max(1u, AlignmentFile::default_threads() / at_once);
        if (!run_file_per_device(S)) return 1;
    } else {
        for (size_t n = 0; n < shared.input_paths.size(); ++n) {
            if (!get_profiles(S, n)) return 1;
            trace.mark("get_profiles + its buffers released");
        }
    }
    closing_lines();
    return 0;
}
