// The window pipeline (include/slimm_hip.h: slimm_push_bam_bytes, _bgzf_blocks, _sam_bytes, _bgzf_sam_blocks, _bzip2_sam_bytes,
// _gzip_sam_bytes, _zstd_sam_bytes, _xz_sam_bytes, _lz4_sam_bytes, _lzip_sam_bytes): a file's bytes -- inflated BAM records, whole BGZF blocks of them, SAM text, BGZF blocks of SAM
// text, SAM text in a streamed codec (bzip2, gzip, zstd, xz, lz4, lzip) -- cross the bus in windows; the device inflates (bgzf_tokens.hip,
// bgzf_inflate.hip) or decodes (the codecs: bzip2_decode.hip, gzip_decode.hip, zstd_decode.hip, xz_decode.hip, lz4_decode.hip, lzip_decode.hip) them, finds the
// records (bam_decode.hip, sam_decode.hip) and appends them to the context's record stream.  Its state: windows.h.
// Replaces seqan::BamFileIn + readRecord of the reference (src/misc.hpp:498-522, src/slimm.hpp:194-208).
// A push's steps (push_window): check_push, open_file; one of three sources fills window buffers -- push_stream (a streamed
// codec: kCodecs says what each supplies), gather_blocks (+ launch_gathered), push_plain --, each window handed over by
// submit_window; finish_windows; release_callers_buffer.
// A window is copied when it is pushed and WORKED ON when the next one is pushed (or at once, when it is the last): its
// host-to-device copy then runs beside the kernels and the host's bookkeeping of the window before it -- the copies are
// what bounds this path (192 MB at 54 GB/s: 3.6 ms; kernels + one synchronisation per window: 0.8 ms).
#include "context.h"

namespace slimm {

void push_trace_line(const char* tag, const char* fmt, va_list ap) {
    static const bool on = traced("push");
    if (!on) return;
    static const auto t0 = std::chrono::steady_clock::now();
    if (tag)
        fprintf(stderr, "[push %s] ", tag);
    else
        fprintf(stderr, "[push %9.3f] ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
}
void push_trace(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    push_trace_line(nullptr, fmt, ap);
    va_end(ap);
}

void WindowPipeline::free_outgrown() {
    for (void* p : outgrown) (void)hipFree(p);
    outgrown.clear();
}

int WindowPipeline::end_file(slimm_ctx* c) {
    if (file.active && file.head < file.windows) {  // a file abandoned with windows in flight (an error, a caller's change
        (void)hipSetDevice(c->device);              // of mind): their copies and inflates must not land in the next file's
        if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));  // buffers
        for (auto& is : inflate_stream)
            if (is) HIP_TRY(c, hipStreamSynchronize(is));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (file.acc_open) {  // (a gathered window that was never launched: its copies)
        (void)hipSetDevice(c->device);
        if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    }
    free_outgrown();
    // (a streamed codec: the next file sizes its own decode scratch; what the host held of this one's bytes goes)
    file = File{};
    announced = Announced{};
    gz_pass = GzipPass{};
    if (held_bytes() > kWindowKeepAcrossFiles) {   // (a large file's windows: the next file sizes its own)
        (void)hipSetDevice(c->device);
        each_held([](auto& b) { b.release(); });
    }
    // (zstd: the page-locked copy of a round's text, for the content checksums, goes with every file: it is no device
    // memory, slimm_window_memory does not count it, and a file without checksums never needs it)
    zst.h_text.release();
    lz.h_text.release();
    return SLIMM_OK;
}

void WindowPipeline::destroy() {
    for (auto& is : inflate_stream)
        if (is) {
            (void)hipStreamSynchronize(is);
            (void)hipStreamDestroy(is);
        }
    if (comp_copied) (void)hipEventDestroy(comp_copied);
    for (auto& r : registered) (void)hipHostUnregister(const_cast<uint8_t*>(r.first));
    free_outgrown();
    for (auto& e : copied)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : h2d_done)
        if (e) (void)hipEventDestroy(e);
}

}  // namespace slimm

namespace {

using File = WindowPipeline::File;
using Codec = File::Codec;
constexpr uint32_t kRing = WindowPipeline::kWindowRing;

// ---- a window is finished.  First, what differs between a window of BAM records and one of SAM lines
uint32_t window_pieces(bool sam, uint64_t n_bytes) { return sam ? sam_pieces(n_bytes) : bam_pieces(n_bytes); }
void launch_find(slimm_ctx* c, const uint8_t* bytes, uint64_t lo, uint64_t end) {
    WindowPipeline& W = c->win;
    if (W.file.sam)
        launch_sam_find(c->stream, bytes, lo, end, W.pieces.p, W.offs.p, W.result.p);
    else
        launch_bam_find(c->stream, bytes, lo, end, c->R, W.pieces.p, W.offs.p, W.result.p);
}
void launch_decode(slimm_ctx* c, const uint8_t* bytes, uint64_t lo, uint64_t end, bool marked) {
    WindowPipeline& W = c->win;
    if (W.file.sam)
        launch_sam_decode(c->stream, bytes, lo, end, W.pieces.p, W.offs.p, W.carry.p, W.result.p, marked, c->n_pushed, c->in_key.p,
                          c->in_ref.p, c->in_pos.p, c->in_flag.p, c->in_check.p, W.sam_table.p, W.sam_mask, W.sam_names.p, W.filter,
                          W.filter_counts.p);
    else
        launch_bam_decode(c->stream, bytes, lo, end, W.pieces.p, W.offs.p, W.carry.p, W.result.p, marked, c->n_pushed, c->in_key.p,
                          c->in_ref.p, c->in_pos.p, c->in_flag.p, c->in_check.p, W.filter, W.filter_counts.p);
}
struct FormTexts { const char *bad, *skipped, *too_long; };
const FormTexts kBamTexts{"bad BAM record", "bad BAM record", "a BAM record longer than 16 MiB: decode this file on the host"};
const FormTexts kSamTexts{"SAM line with fewer than 10 fields", "a header line or an empty line among the alignment lines: decode this file on the host",
                          "a SAM line longer than 16 MiB: decode this file on the host"};
// what the inflate of the window in buffer b reported (fetched into h_inflate_status)
int check_inflate(slimm_ctx* c) {
    const uint32_t* s = c->win.h_inflate_status.p;
    if (s[0]) return fail(c, SLIMM_E_INVALID, "corrupt BGZF block (device inflate: error %u in block %u of the window)", s[0], s[1]);
    return SLIMM_OK;
}

// A range that starts inside the file (slimm_set_input_mid_file): its first record is guessed from the bytes of its first
// window, as k_bam_pieces guesses a piece's; the bytes in front of it (the head, at most 16 MiB) stay on the device for the
// member on the left, which confirms the guess (slimm_group_stitch_ranges).  No record start at all: the whole window is
// head (a range inside one long record) -- only when it is the range's last window.  lo: where the window's records start
//
// SAM text: the first line starts behind the first newline, and the head is the bytes through that newline -- a whole
// line when the cut fell on a line start; nothing is guessed, and the member on the left checks only that its last line
// ends with the head.
int guess_first_record(slimm_ctx* c, uint32_t b, uint64_t n_bytes, bool is_last, uint64_t end, uint64_t& lo) {
    WindowPipeline& W = c->win;
    hipStream_t st = c->stream;
    if (n_bytes) HIP_TRY(c, hipStreamWaitEvent(st, W.copied[b], 0));
    HIP_TRY(c, W.guess.ensure(1));
    HIP_TRY(c, hipMemsetAsync(W.guess.p, 0xff, sizeof(unsigned long long), st));
    if (W.file.sam)
        launch_sam_first_newline(st, W.bytes[b].p, lo, std::min<uint64_t>(end, lo + kBamSlack), W.guess.p);
    else
        launch_bam_first_guess(st, W.bytes[b].p, lo, std::min<uint64_t>(end, lo + kBamSlack + 1u), end, c->R, W.guess.p);
    unsigned long long g = 0;
    HIP_TRY(c, hipMemcpyAsync(&g, W.guess.p, sizeof(g), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    W.file.found_start = g != ~0ull;
    if (!W.file.found_start) {
        if (!is_last || end - lo > kBamSlack)
            return fail(c, SLIMM_E_SPLIT, "no %s starts in the first 16 MiB of a range that starts inside the file", W.file.sam ? "line" : "record");
        g = end;
    } else if (W.file.sam) {
        ++g;   // (the line starts behind the newline)
    }
    const uint64_t head = g - lo;
    HIP_TRY(c, W.head_bytes.ensure(std::max<uint64_t>(head + 64u, 4096u)));
    if (head) HIP_TRY(c, hipMemcpyAsync(W.head_bytes.p, W.bytes[b].p + lo, head, hipMemcpyDeviceToDevice, st));
    W.file.head_len = head;
    // (SLIMM_FORCE split_shift_guess: the join sees a guess one byte off, and must refuse it)
    if (W.file.found_start && forced("split_shift_guess")) W.file.head_len = head ? head - 1u : 1u;
    lo = g;
    return SLIMM_OK;
}

// The text's last bytes were inflated here: the host could not give a last line without its newline one, the device does
// (status word 3 of the buffer: the line was ended) -- `end` moves behind it
int end_last_line_on_device(slimm_ctx* c, uint64_t j, uint32_t b, uint64_t lo, bool inflated_here, uint64_t& end) {
    WindowPipeline& W = c->win;
    hipStream_t st = c->stream;
    launch_sam_end_line(st, W.bytes[b].p, lo, end, W.inflate_status.p + 4u * b + 3u);
    HIP_TRY(c, hipMemcpyAsync(W.h_inflate_status.p, W.inflate_status.p + 4u * b, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (inflated_here && check_inflate(c) != SLIMM_OK) return SLIMM_E_INVALID;
    if (W.h_inflate_status.p[3]) {
        ++W.file.sam_lines_ended;
        push_trace("window %llu: the text's last line ended on the device", (unsigned long long)j);
    }
    end += W.h_inflate_status.p[3];
    return SLIMM_OK;
}

// window j (n bytes, in buffer j % kWindowRing) -> records appended; the incomplete record at its end goes in front of window j + 1
int finish_window(slimm_ctx* c, uint64_t j, uint64_t n_bytes, bool is_last, uint64_t& n_rec_out) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    hipStream_t st = c->stream;
    const bool marked = c->order == SLIMM_ORDER_GROUPED;
    const FormTexts& texts = F.sam ? kSamTexts : kBamTexts;
    const uint32_t b = static_cast<uint32_t>(j % kRing), nb = static_cast<uint32_t>((j + 1u) % kRing);
    uint64_t lo = kBamSlack - F.carry_bytes;
    uint64_t end = kBamSlack + n_bytes;
    if (n_bytes) HIP_TRY(c, hipStreamWaitEvent(st, W.copied[b], 0));
    const bool inflated_here = n_bytes && F.inflated[b];
    // (a range that ends inside the file ends inside a line: that line is the carry, and the member on the right ends it)
    if (F.sam && is_last && F.sam_dev_tail && !W.announced.ends_mid) SLIMM_TRY(end_last_line_on_device(c, j, b, lo, inflated_here, end));
    if (W.announced.starts_mid && j == 0) SLIMM_TRY(guess_first_record(c, b, n_bytes, is_last, end, lo));
    const uint32_t np = window_pieces(F.sam, end - lo);
    // (with room to spare and without a hipFree: windows differ by a few pieces, and a hipFree waits for the inflate kernels
    // of the windows behind this one)
    if (W.pieces.cap < static_cast<size_t>(np) + 1) HIP_TRY(c, W.pieces.ensure_later(static_cast<size_t>(np) + (np >> 2) + 64, W.outgrown));
    if (W.offs.cap < static_cast<size_t>(np + 1) * kBamSlots)
        HIP_TRY(c, W.offs.ensure_later((static_cast<size_t>(np) + (np >> 2) + 64) * kBamSlots, W.outgrown));
    if (inflated_here)
        HIP_TRY(c, hipMemcpyAsync(W.h_inflate_status.p, W.inflate_status.p + 4u * b, 16, hipMemcpyDeviceToHost, st));
    launch_find(c, W.bytes[b].p, lo, end);
    HIP_TRY(c, hipStreamSynchronize(st));  // the window is on the device and counted
    if (inflated_here && check_inflate(c) != SLIMM_OK) return SLIMM_E_INVALID;
    const BamWindowResult res = *W.result.p;
    if (res.bad) return fail(c, SLIMM_E_INVALID, "%s", (res.bad & kBamPieceBad) ? texts.bad : texts.skipped);
    const uint64_t n_rec = res.n_records, stop = np ? res.stop : end;
    const uint64_t tail = end - stop;
    if (tail > kBamSlack) return fail(c, SLIMM_E_INVALID, "%s", texts.too_long);
    if (is_last && tail && !W.announced.ends_mid) return fail(c, SLIMM_E_INVALID, "truncated BAM record");
    if (c->n_pushed + n_rec >= record_cap()) return fail(c, SLIMM_E_INVALID, "a context handles fewer than 2^31 records; shard the stream");
    SLIMM_TRY(slimm_reserve(c, c->n_pushed + n_rec));
    const uint64_t want = c->n_pushed + n_rec;
    if (!marked && (c->in_flag.cap < want || c->in_check.cap < want)) {  // (the four-array form's flag and check arrays
        if (c->n_pushed) return fail(c, SLIMM_E_HIP, "record arrays out of step");   // appear at a file's first window)
        if (c->in_flag.cap < want) HIP_TRY(c, c->in_flag.ensure_later(std::max<uint64_t>(want, c->in_ref.cap), W.outgrown));
        if (c->in_check.cap < want) HIP_TRY(c, c->in_check.ensure_later(std::max<uint64_t>(want, c->in_ref.cap), W.outgrown));
    }
    launch_decode(c, W.bytes[b].p, lo, end, marked);
    if (W.announced.starts_mid && !F.has_first && n_rec) {   // (the range's first record: a window's first record starts at lo)
        HIP_TRY(c, W.first.ensure(1));
        if (F.sam)
            launch_sam_name_at(st, W.bytes[b].p, lo, end, W.first.p);
        else
            launch_bam_name_at(st, W.bytes[b].p, lo, W.first.p);
        F.has_first = true;
    }
    if (tail) {  // the incomplete record goes in front of the next window (whose own bytes may be on their way already)
        if (W.bytes[nb].cap < kBamSlack + 64) HIP_TRY(c, W.bytes[nb].ensure(kBamSlack + 64));
        HIP_TRY(c, hipMemcpyAsync(W.bytes[nb].p + kBamSlack - tail, W.bytes[b].p + stop, tail, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(c, hipGetLastError());
    F.carry_bytes = tail;
    c->n_pushed += n_rec;
    view_records(c);
    n_rec_out = n_rec;
    return SLIMM_OK;
}

// The oldest windows finished (found, counted, decoded), their records added to total: while more than kWindowLag windows or
// kWindowInFlight bytes are in flight, or all of them.  last: the newest window is the file's last
enum class Upto { Lag, All };
int finish_windows(slimm_ctx* c, Upto upto, bool last, bool trace, uint64_t& total) {
    File& F = c->win.file;
    while (F.head < F.windows) {
        uint64_t in_flight = 0;
        for (uint64_t j = F.head; j < F.windows; ++j) in_flight += F.win_bytes[j % kRing];
        if (upto == Upto::Lag && F.windows - F.head <= WindowPipeline::kWindowLag && in_flight <= WindowPipeline::kWindowInFlight) break;
        uint64_t got = 0, j = F.head;
        if (trace)
            push_trace("finishing window %llu (%llu .. %llu in flight, %.0f MB)", (unsigned long long)j, (unsigned long long)F.head,
                       (unsigned long long)F.windows, in_flight / 1e6);
        const int rc = finish_window(c, j, F.win_bytes[j % kRing], last && j + 1 == F.windows, got);
        if (trace) push_trace("finished window %llu: %llu records", (unsigned long long)j, (unsigned long long)got);
        ++F.head;
        if (rc != SLIMM_OK) return rc;
        total += got;
    }
    return SLIMM_OK;
}

// ---- a window is handed over
uint32_t next_buffer(const File& F) { return static_cast<uint32_t>(F.windows % kRing); }

// the window buffer of window `windows`, large enough for n_bytes behind its slack; what the slack holds is kept
int window_buffer(slimm_ctx* c, uint64_t n_bytes, bool gathered = false) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    const uint32_t b = next_buffer(F);
    // (a gathered window gets the room of the largest one at once: a buffer that grows is a hipFree, and a hipFree waits for
    // the inflate kernels of the windows before)
    // (planned from the caller's hint; not told: a quarter more than this window needs, up to the largest window there is)
    const uint64_t room = !gathered    ? n_bytes
                          : F.win_cap ? std::max<uint64_t>(n_bytes, F.win_cap)
                                      : std::max<uint64_t>(n_bytes, std::min<uint64_t>(WindowPipeline::kWindowGather, n_bytes + (n_bytes >> 2)));
    const uint64_t need = kBamSlack + room + 64;
    if (W.bytes[b].cap >= need) return SLIMM_OK;
    // (what the buffer held -- the window a ring's length back -- is done with: it was finished before this one was let in.
    // Only the carried bytes in its slack matter, and only when the window before this one is finished already: otherwise
    // its end will put them there later)
    if (F.head == F.windows && F.carry_bytes)
        HIP_TRY(c, W.bytes[b].grow_keeping(need + (need >> 3), kBamSlack - F.carry_bytes, F.carry_bytes, c->stream, true, &W.outgrown));
    else
        HIP_TRY(c, W.bytes[b].ensure_later(need + (gathered ? 0u : need >> 3), W.outgrown));
    return SLIMM_OK;
}

// Buffer `windows % kWindowRing` now holds window `windows`, n_bytes of it behind the slack: the window's event goes behind
// the work that puts them there (on `filled_on`), and the window is in flight
int submit_window(slimm_ctx* c, uint64_t n_bytes, hipStream_t filled_on, bool inflated_here, bool record_event = true) {
    WindowPipeline& W = c->win;
    const uint32_t b = next_buffer(W.file);
    if (record_event) HIP_TRY(c, hipEventRecord(W.copied[b], filled_on));
    W.file.inflated[b] = inflated_here;
    W.file.win_bytes[b] = n_bytes;
    ++W.file.windows;
    return SLIMM_OK;
}

// SAM text whose last line has no newline gets one: a line ends where its newline is.  (When the text's last bytes were
// inflated on the device, the host has not seen them: finish_window lets the device end that line.  A range that ends
// inside the file -- slimm_set_input_mid_file -- ends inside a line: nothing ends it here)
bool lacks_last_newline(const slimm_ctx* c, bool last) {
    const File& F = c->win.file;
    return F.sam && last && !c->win.announced.ends_mid && !F.sam_dev_tail && F.sam_last_byte != '\n';
}
int add_last_newline(slimm_ctx* c, uint64_t at, hipStream_t st) {   // at: bytes of the next window in front of it
    HIP_TRY(c, hipMemsetAsync(c->win.bytes[next_buffer(c->win.file)].p + kBamSlack + at, '\n', 1, st));
    c->win.file.sam_last_byte = '\n';
    return SLIMM_OK;
}

// ---- a push
enum { kFormatBam = 0, kFormatBgzf = 1, kFormatSam = 2, kFormatBgzfSam = 3, kFormatBzip2Sam = 4, kFormatGzipSam = 5, kFormatZstdSam = 6, kFormatXzSam = 7, kFormatLz4Sam = 8, kFormatLzipSam = 9 };

// What each streamed codec supplies (windows.h: StreamCodec), by File::Codec
const StreamCodec kCodecs[] = {
    {},
    // (ended: the range's chain has stopped, what comes now are bytes of the slack.  Every row's last line: its split side)
    {"bzip2", "bzip2_round", 32ull << 20, true, false, bz2_decode_batch, bz2_next_window, bz2_emit, nullptr, bz2_trace_file, nullptr,
     [](const File& F) { return F.bz2.chain.ended; }, nullptr, 0, 0, nullptr, nullptr,
     true, split_bz2_chains, "cut in front of member %u: %s", "the chain of blocks across a cut", nullptr},
    {"gzip", "gzip_round", 32ull << 20, false, false, gz_round, gz_next_window, gz_emit, nullptr, gz_trace_file,
     [](const File& F) { return static_cast<int>(F.gz.stage); }, nullptr, [](WindowPipeline& W) { return W.gz_stats; },
     WindowPipeline::kGzStats, WindowPipeline::kGzCompressed, nullptr, nullptr,
     false, split_gz_chains, "the range of member %u: %s", "a gzip member across a cut", split_gz_windows},
    {"zstd", "zstd_round", kZstdRoundBytes, true, true, zs_round, zs_next_window, zs_emit, zs_check, zs_trace_file,
     [](const File& F) { return static_cast<int>(F.zst.walk.stage); }, nullptr, [](WindowPipeline& W) { return W.zs_stats; },
     WindowPipeline::kZsStats, WindowPipeline::kZsCompressedBytes, nullptr, nullptr,
     false, split_zstd_ends, "the range of member %u: %s", "the frames of a range", nullptr},
    {"xz", "xz_round", 32ull << 20, true, true, xz_round, xz_next_window, xz_emit, nullptr, xz_trace_file,
     [](const File& F) { return static_cast<int>(F.xz.walk.stage); }, nullptr, [](WindowPipeline& W) { return W.xz_stats; },
     WindowPipeline::kXzStats, WindowPipeline::kXzCompressedBytes, "an", "block",
     true, split_xz_streams, "the range of member %u: %s", "the blocks of a stream across a cut", nullptr},
    // (not cut by byte range: no split side)
    {"lz4", "lz4_round", kLz4RoundBytes, false, false, lz4_round, lz4_next_window, lz4_emit, lz4_check, lz4_trace_file,
     [](const File& F) { return static_cast<int>(F.lz.walk.stage); }, nullptr, [](WindowPipeline& W) { return W.lz_stats; },
     WindowPipeline::kLzStats, WindowPipeline::kLzCompressedBytes, "an", nullptr,
     false, nullptr, nullptr, nullptr, nullptr},
    // (not cut by byte range: no split side.  Its rounds go on while the file offset moves: the members taken)
    {"lzip", "lzip_round", kLzipRoundBytes, false, false, lzip_round, lzip_next_window, lzip_emit, nullptr, lzip_trace_file,
     [](const File&) { return 0; }, nullptr, [](WindowPipeline& W) { return W.lzip_stats; },
     WindowPipeline::kLzipStats, WindowPipeline::kLzipCompressedBytes, "an", nullptr,
     false, nullptr, nullptr, nullptr, nullptr},
};

struct Push {
    const uint8_t* bytes;
    uint64_t src_bytes, n_bytes;   // what crosses the bus; the push's record bytes (text bytes)
    uint32_t skip;                 // inflated (a streamed codec: decoded) bytes in front of the file's first record
    bool last, sam;
    Codec codec;                   // a streamed codec's SAM: the file's bytes, decoded here
    bool compressed;               // BGZF blocks to inflate here: their descriptors, their inflated bytes
    std::vector<BgzfBlock> blocks = {};
    uint64_t inflated = 0;
    bool copy_started = false;     // this push started a copy from the caller's buffer
};

// BGZF blocks: their descriptors; the blocks in front of the file's first record dropped, `skip` what is left of them
int trim_bgzf_push(slimm_ctx* c, Push& p) {
    if (!p.src_bytes) p.compressed = false;
    if (!p.compressed) return SLIMM_OK;
    const File& F = c->win.file;
    std::vector<BgzfBlock>& dh = p.blocks;
    if (!p.bytes) return fail(c, SLIMM_E_INVALID, "null byte buffer");
    std::string why;
    if (!bgzf_parse_blocks(p.bytes, p.src_bytes, 0, dh, p.inflated, why)) return fail(c, SLIMM_E_INVALID, "%s", why.c_str());
    if (p.skip > p.inflated || (p.skip && F.active && (F.windows > 0 || F.acc_open)))
        return fail(c, SLIMM_E_INVALID, "skip: only in front of a file's first records");
    if (dh.size() >= (1ull << 31)) return fail(c, SLIMM_E_INVALID, "too many blocks in one window");
    p.n_bytes = p.inflated - p.skip;
    // blocks that lie wholly inside the skipped bytes (a BAM header of any size) are not inflated at all; what is left to
    // skip is less than one block, so the inflater's first byte stays inside the window buffer's slack
    size_t drop = 0;
    while (drop < dh.size() && dh[drop].dst + dh[drop].isize <= p.skip) ++drop;
    if (drop) {
        const uint64_t d0 = drop < dh.size() ? dh[drop].dst : p.inflated;
        dh.erase(dh.begin(), dh.begin() + static_cast<long>(drop));
        for (BgzfBlock& d : dh) d.dst -= d0;
        p.skip -= static_cast<uint32_t>(d0);
        p.inflated -= d0;
    }
    if (p.skip >= 65536u) return fail(c, SLIMM_E_INVALID, "skip: past the first block that holds a record byte");
    if (p.n_bytes == 0) {  // (blocks without a record byte: nothing to inflate, nothing to decode)
        p.compressed = false;
        p.src_bytes = 0;
    }
    return SLIMM_OK;
}

// The call against the context and the file so far, in this order: a call that is wrong in two ways reports the first
int check_push(slimm_ctx* c, Push& p) {
    const File& F = c->win.file;
    if (p.sam && !c->win.sam_mask) return fail(c, SLIMM_E_INVALID, "slimm_set_reference_names first: SAM text names its references");
    if (F.active && F.sam != p.sam) return fail(c, SLIMM_E_INVALID, "SAM text and BAM bytes do not mix within a file");
    const Codec mine = F.stream.codec, named = mine == Codec::None ? p.codec : p.codec == Codec::None ? mine : std::min(mine, p.codec);
    const StreamCodec& K = codec_of(p.codec);
    const bool mid = c->win.announced.starts_mid || c->win.announced.ends_mid;
    if (F.active && mine != p.codec)   // (two codecs: the text names the first of them in Codec's order)
        return fail(c, SLIMM_E_INVALID, "%s SAM bytes and the other forms do not mix within a file", codec_of(named).name);
    const bool gz_range = p.codec == Codec::Gzip && c->win.announced.gz_range;   // (gzip is cut at announced bits only)
    if (K.name && !K.cut_by_range && mid && !gz_range) return fail(c, SLIMM_E_INVALID, "%s %s stream is not cut by byte range", K.article ? K.article : "a", K.name);
    if (K.name && K.cut_at_frames && mid && !c->win.announced.has_range)
        return fail(c, SLIMM_E_INVALID, "%s %s stream is not cut by byte range unless its range is announced (slimm_set_input_range) and starts at a %s",
                    K.article ? K.article : "a", K.name, K.cut_unit ? K.cut_unit : "frame");
    if (K.name && p.skip && F.active) return fail(c, SLIMM_E_INVALID, "skip: only in front of a file's first records");
    if (K.name && K.cut_by_range && !F.active && mid && !c->win.announced.has_range)
        return fail(c, SLIMM_E_INVALID, "slimm_set_input_range first: a range of a %s file is cut at bits, told by where it lies in the file", K.name);
    SLIMM_TRY(trim_bgzf_push(c, p));
    if (c->device < 0) return fail(c, SLIMM_E_INVALID, "host-only context has no record stream");
    if (p.n_bytes && !p.bytes) return fail(c, SLIMM_E_INVALID, "null byte buffer");
    if (c->analyzed) return fail(c, SLIMM_E_INVALID, "records already analysed; reset first");
    if (c->borrowed) return fail(c, SLIMM_E_INVALID, "records are borrowed device arrays; reset first");
    if (p.n_bytes >= (1ull << 31)) return fail(c, SLIMM_E_INVALID, "a window of BAM bytes is less than 2 GiB");
    if (c->n_pushed && !F.active)
        return fail(c, SLIMM_E_INVALID, "earlier batches were decoded records: the forms do not mix within a file");
    if (F.closed) return fail(c, SLIMM_E_INVALID, "the file's last window has been pushed; reset first");
    return SLIMM_OK;
}

// A file's first window: its form, the record form it decodes to, and what every window needs (the state itself is fresh:
// WindowPipeline::end_file)
int open_file(slimm_ctx* c, const Push& p) {
    WindowPipeline& W = c->win;
    if (W.file.active) return SLIMM_OK;
    const bool marked = c->order == SLIMM_ORDER_GROUPED;
    W.file.active = true;
    W.file.sam = p.sam;
    const StreamCodec& K = codec_of(p.codec);
    W.file.stream.codec = p.codec;
    W.file.stream.skip_left = K.name ? p.skip : 0u;
    if (K.stats) std::fill(K.stats(W), K.stats(W) + K.n_stats, 0ull);
    if (K.cut_by_range && W.announced.has_range) W.file.stream.base = W.announced.range_begin;   // (errors name the file's bytes)
    if (p.codec == Codec::Gzip && W.announced.gz_range) {
        const WindowPipeline::Announced& A = W.announced;
        File::Gzip& Z = W.file.gz;
        W.file.stream.base = A.gz_begin_bit >> 3;
        Z.window_pass = A.gz_window_pass;
        if (A.starts_mid) {   // (among a member's blocks: no header is expected, and its trailer is not this range's to check)
            W.file.stream.bit = A.gz_begin_bit & 7u;
            Z.stage = File::Gzip::Deflate;
            Z.partial = true;
            Z.crc = 0;
            Z.front = Z.window_pass || !W.gz_pass.has_front ? gz::kWindow : W.gz_pass.front_len;
        }
    }
    c->marked = marked;
    c->has_check = !marked;
    c->packed = false;
    HIP_TRY(c, W.carry.ensure(1));
    HIP_TRY(c, W.result.ensure(1));
    for (auto& e : W.copied)
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : W.h2d_done)
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(c, hipMemsetAsync(W.carry.p, 0, sizeof(BamCarry), c->stream));
    if (slimm_rf_on(&W.filter)) {
        HIP_TRY(c, W.filter_counts.ensure(SLIMM_RF_N_STATS));
        HIP_TRY(c, hipMemsetAsync(W.filter_counts.p, 0, SLIMM_RF_N_STATS * sizeof(uint32_t), c->stream));
        W.file.filter_counted = true;
    }
    return SLIMM_OK;
}

// A streamed codec: the bytes wait on the host until a round's worth has come (or the file ends); then round by round what
// can be decoded of them is (the codec's decoder), and each round's text becomes a window of its own -- or several, where
// the codec cuts it (bzip2: a batch of blocks)
int push_stream(slimm_ctx* c, const Push& p, uint64_t& total) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    File::Stream& S = F.stream;
    const StreamCodec& K = codec_of(p.codec);
    hipStream_t st = c->stream;
    if (p.n_bytes && !(K.ended && K.ended(F))) {
        S.pend.insert(S.pend.end(), p.bytes, p.bytes + p.n_bytes);
        S.found = S.waiting = false;
        if (K.stats) K.stats(W)[K.stat_compressed] += p.n_bytes;
    }
    long round = 0;
    if (!forced(K.round_key, &round) || round <= 0) round = static_cast<long>(K.round_bytes);
    const bool decode_now = p.last || S.pend.size() - (S.bit >> 3) >= static_cast<uint64_t>(round);
    while (decode_now) {
        // (the one moment the bytes read so far go: a round's start, unless the device holds pend as it is and the round
        // goes on in those bytes)
        if (!S.found) S.drop_read();
        const uint64_t at0 = S.base * 8u + S.bit;
        const int stage0 = K.stage ? K.stage(F) : 0;
        SLIMM_TRY(K.round(c, p.last));
        uint64_t n = 0;
        bool any = false;
        for (; K.next_window(c, WindowPipeline::kWindowGather, &n); any = true) {
            SLIMM_TRY(window_buffer(c, n + 1u));
            uint8_t lb = '\n';
            SLIMM_TRY(K.emit(c, W.bytes[next_buffer(F)].p + kBamSlack, WindowPipeline::kWindowGather, &n, &lb));
            if (n) {   // (none: a round of header only)
                F.sam_last_byte = lb;
                SLIMM_TRY(submit_window(c, n, st, false));
                push_trace("window %llu: %.1f MB of text from %s", (unsigned long long)(F.windows - 1), n / 1e6, K.name);
            }
            if (K.behind_submit) SLIMM_TRY(K.behind_submit(c));
            if (n) SLIMM_TRY(finish_windows(c, Upto::Lag, false, false, total));
        }
        if (K.stage ? S.waiting || (S.base * 8u + S.bit == at0 && K.stage(F) == stage0) : !any) break;
    }
    if (lacks_last_newline(c, p.last)) {   // (in a window of its own)
        SLIMM_TRY(window_buffer(c, 1u));
        SLIMM_TRY(add_last_newline(c, 0, st));
        SLIMM_TRY(submit_window(c, 1, st, false));
    }
    if (p.last) K.trace_file(c);
    return SLIMM_OK;
}

// A file's first compressed push: the buffers its windows will take in turn, now -- an allocation (like a hipFree) made while
// inflate kernels are in flight waits for them, and the pushes that should overlap them stand still.  How many and how large
// comes from the caller's hint (slimm_set_input_size_hint: the file's compressed bytes) and this push's own ratios: a 70 MB
// file gets one window of its size, not four of 1.9 GB (17 GB per context whatever the file).  Without a hint
// nothing is reserved ahead: buffers appear as windows need them.
// (windows the host inflated may have gone before this push: they are finished first -- their buffers are about to be
// replaced; the bytes they carry over move with the buffer of the window that is next)
int plan_file_buffers(slimm_ctx* c, const Push& p, uint64_t& total) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    const uint64_t size_hint = W.announced.size_hint, gather = WindowPipeline::kWindowGather, goal = WindowPipeline::kWindowGatherGoal;
    F.planned = true;
    F.win_cap = 0;
    if (!size_hint || !p.src_bytes || !p.inflated) return SLIMM_OK;
    SLIMM_TRY(finish_windows(c, Upto::All, false, false, total));
    const double ratio = static_cast<double>(p.inflated) / static_cast<double>(p.src_bytes);
    const uint64_t left = size_hint > p.src_bytes ? size_hint - p.src_bytes : 0;
    const uint64_t est = p.inflated + static_cast<uint64_t>(static_cast<double>(left) * ratio * 1.08) + (16ull << 20);
    const uint64_t nwin = est <= gather ? 1u : (est + goal - 1) / goal;
    const uint32_t nbuf = static_cast<uint32_t>(std::min<uint64_t>(kRing, nwin));
    F.win_cap = nwin == 1 ? est : gather;
    // (a window's compressed bytes: what inflates to the goal, plus the push that crosses it)
    const uint64_t comp_cap = (nwin == 1 ? size_hint + (size_hint >> 4) : static_cast<uint64_t>(static_cast<double>(goal) / ratio * 1.15) + p.src_bytes) +
                              kBgzfTail + (1ull << 20);
    const double blocks_per_byte = static_cast<double>(p.blocks.size()) / static_cast<double>(p.inflated);
    const uint32_t blocks_max = static_cast<uint32_t>(static_cast<double>(F.win_cap) * blocks_per_byte * 1.25) + 1024u;
    const uint64_t tok_max = F.win_cap / 3u + F.win_cap / 256u + 8ull * blocks_max;
    for (uint32_t k = 0; k < nbuf; ++k) {
        if (k == next_buffer(F) && F.carry_bytes) {   // (the carried bytes lie in this buffer's slack: window_buffer keeps them)
            SLIMM_TRY(window_buffer(c, F.win_cap, true));
        } else {
            HIP_TRY(c, W.bytes[k].ensure_later(kBamSlack + F.win_cap + 64, W.outgrown));
        }
        HIP_TRY(c, W.comp[k].ensure_later(comp_cap, W.outgrown));
        HIP_TRY(c, W.desc[k].ensure_later(blocks_max, W.outgrown));
    }
    for (uint32_t k = 0; k < std::min<uint32_t>(2u, nbuf); ++k)
        HIP_TRY(c, W.inflate_scratch[k].ensure_later(bgzf_inflate_scratch_bytes(blocks_max, tok_max), W.outgrown));
    const size_t np_max = window_pieces(p.sam, F.win_cap + kBamSlack) + 64;
    HIP_TRY(c, W.pieces.ensure_later(np_max, W.outgrown));
    HIP_TRY(c, W.offs.ensure_later(np_max * kBamSlots, W.outgrown));
    push_trace("buffers reserved");
    push_trace("planned %llu window(s) of <= %.0f MB in %u buffer(s), %.0f MB of compressed bytes each: %.2f GB held",
               (unsigned long long)nwin, F.win_cap / 1e6, nbuf, comp_cap / 1e6, W.held_bytes() / 1e9);
    return SLIMM_OK;
}

// The BGZF blocks gathered so far become window `windows`: descriptors over, the inflate launched behind the copies on the
// inflate stream whose turn it is.
int launch_gathered(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    if (!F.acc_open) return SLIMM_OK;
    const uint32_t b = next_buffer(F), si = static_cast<uint32_t>(F.windows & 1u);
    const uint32_t nblk = static_cast<uint32_t>(W.desc_host[b].size());
    const uint64_t n_bytes = F.acc_dst - F.acc_skip;
    F.acc_open = false;
    if (!nblk || !n_bytes) return SLIMM_OK;
    SLIMM_TRY(window_buffer(c, n_bytes, true));
    // (room to spare only when a buffer has to GROW: a request "with a quarter more" that exceeded a buffer reserved for exactly
    // this kind of window re-allocated 3 GB of scratch in the middle of a file -- a hipMalloc that waits for the kernels in
    // flight and, now and then, 1.4 s for the memory itself: profiles/round6/06_cli_stall_hunt.txt)
    if (W.desc[b].cap < static_cast<size_t>(nblk) + 1)
        HIP_TRY(c, W.desc[b].ensure_later(static_cast<size_t>(nblk) + (nblk >> 1) + 1, W.outgrown));
    if (W.inflate_scratch[si].cap < bgzf_inflate_scratch_bytes(nblk, F.acc_tok)) {
        push_trace("inflate scratch %u grows: %.0f MB held, %.0f MB needed", si, W.inflate_scratch[si].cap / 1e6,
                   bgzf_inflate_scratch_bytes(nblk, F.acc_tok) / 1e6);
        HIP_TRY(c, W.inflate_scratch[si].ensure_later(bgzf_inflate_scratch_bytes(nblk + (nblk >> 2), F.acc_tok + (F.acc_tok >> 2)), W.outgrown));
    }
    HIP_TRY(c, W.inflate_status.ensure(4u * kRing));
    HIP_TRY(c, W.h_inflate_status.ensure(4));
    HIP_TRY(c, hipMemsetAsync(W.comp[b].p + F.acc_src, 0, kBgzfTail, c->copy_stream));
    HIP_TRY(c, hipMemcpyAsync(W.desc[b].p, W.desc_host[b].data(), static_cast<size_t>(nblk) * sizeof(BgzfBlock), hipMemcpyHostToDevice,
                              c->copy_stream));
    HIP_TRY(c, hipMemsetAsync(W.inflate_status.p + 4u * b, 0, 16, c->copy_stream));
    HIP_TRY(c, hipMemsetAsync(W.inflate_status.p + 4u * b + 1u, 0xff, 4, c->copy_stream));
    HIP_TRY(c, need_stream(W.inflate_stream[si], kStreamLow));
    if (!W.comp_copied) HIP_TRY(c, hipEventCreateWithFlags(&W.comp_copied, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(W.comp_copied, c->copy_stream));
    HIP_TRY(c, hipStreamWaitEvent(W.inflate_stream[si], W.comp_copied, 0));
    launch_bgzf_inflate(W.inflate_stream[si], W.comp[b].p, W.desc[b].p, nblk, W.bytes[b].p + kBamSlack - F.acc_skip, W.inflate_scratch[si].p,
                        W.inflate_status.p + 4u * b);
    SLIMM_TRY(submit_window(c, n_bytes, W.inflate_stream[si], true));
    push_trace("window %llu launched: %u blocks, %.0f MB -> %.0f MB, inflate stream %u", (unsigned long long)(F.windows - 1), nblk,
               F.acc_src / 1e6, n_bytes / 1e6, si);
    return SLIMM_OK;
}

// BGZF pushes are GATHERED: their compressed bytes are copied behind each other into the next window's buffer, and the window
// is launched -- inflate, then the record kernels -- once it holds kWindowGatherGoal inflated bytes (or the file ends, or a
// push of the other kind comes): the inflate's first phase is a lane per block and wants tens of thousands of them, whatever
// size the caller's buffers have.
int gather_blocks(slimm_ctx* c, Push& p, uint64_t& total) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    // behind what is gathered already -- unless the window would grow past its size: that one goes first
    if (F.acc_open && F.acc_dst + p.inflated > WindowPipeline::kWindowGather) {
        SLIMM_TRY(launch_gathered(c));
    }
    const uint32_t b = next_buffer(F);
    if (!F.acc_open) {
        F.acc_open = true;
        F.acc_src = F.acc_dst = 0;
        F.acc_skip = p.skip;
        F.acc_tok = 0;
        W.desc_host[b].clear();
        if (!F.planned) {
            SLIMM_TRY(plan_file_buffers(c, p, total));
            HIP_TRY(c, W.inflate_status.ensure(4u * kRing));
            HIP_TRY(c, W.h_inflate_status.ensure(4));
        }
    }
    const uint64_t need = F.acc_src + p.src_bytes + kBgzfTail + 64;
    // (grown with what earlier pushes of this window have put there; no hipFree here: it would wait for the inflate kernels in flight)
    if (W.comp[b].cap < need) HIP_TRY(c, W.comp[b].grow_keeping(need + (need >> 1), 0, F.acc_src, c->copy_stream, false, &W.outgrown));
    HIP_TRY(c, hipMemcpyAsync(W.comp[b].p + F.acc_src, p.bytes, p.src_bytes, hipMemcpyHostToDevice, c->copy_stream));
    HIP_TRY(c, hipEventRecord(W.h2d_done[F.pushes % 4u], c->copy_stream));
    ++F.pushes;
    p.copy_started = true;
    const uint32_t tok0 = p.blocks.empty() ? 0u : p.blocks.front().tok;   // (blocks dropped in front of a file's first record)
    for (BgzfBlock& d : p.blocks) {
        d.src += F.acc_src;
        d.dst += F.acc_dst;
        d.tok = d.tok - tok0 + F.acc_tok;
    }
    if (!p.blocks.empty()) F.acc_tok = p.blocks.back().tok + bgzf_token_room(p.blocks.back().isize);
    W.desc_host[b].insert(W.desc_host[b].end(), p.blocks.begin(), p.blocks.end());
    F.acc_src += p.src_bytes;
    F.acc_dst += p.inflated;
    F.sam_dev_tail = p.sam;   // (the text's last bytes so far are the device's to see)
    if (F.acc_dst >= WindowPipeline::kWindowGatherGoal) return launch_gathered(c);
    return SLIMM_OK;
}

// inflated bytes / text: a window of their own, behind what was gathered.  (An empty last window goes behind text whose last
// bytes were inflated on the device: finish_window ends that line there)
int push_plain(slimm_ctx* c, Push& p) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    SLIMM_TRY(launch_gathered(c));
    if (p.sam && p.n_bytes) {
        F.sam_last_byte = p.bytes[p.n_bytes - 1];
        F.sam_dev_tail = false;
    }
    const bool add_newline = lacks_last_newline(c, p.last);
    SLIMM_TRY(window_buffer(c, p.n_bytes + (add_newline ? 1u : 0u)));
    const uint64_t n = p.n_bytes;
    if (n) HIP_TRY(c, hipMemcpyAsync(W.bytes[next_buffer(F)].p + kBamSlack, p.bytes, n, hipMemcpyHostToDevice, c->copy_stream));
    if (add_newline) SLIMM_TRY(add_last_newline(c, n, c->copy_stream));
    SLIMM_TRY(submit_window(c, n + (add_newline ? 1u : 0u), c->copy_stream, false));
    HIP_TRY(c, hipEventRecord(W.h2d_done[F.pushes % 4u], c->copy_stream));
    ++F.pushes;
    p.copy_started = true;
    return SLIMM_OK;
}

// the caller's buffer of the call BEFORE this one has been read (it may be reused once this call returns): the most recent
// push whose copy this call did not start itself (a call without record bytes starts none)
int release_callers_buffer(slimm_ctx* c, const Push& p) {
    WindowPipeline& W = c->win;
    const uint64_t mine = p.copy_started ? 1u : 0u;
    if (W.file.pushes > mine) HIP_TRY(c, hipEventSynchronize(W.h2d_done[(W.file.pushes - 1u - mine) % 4u]));
    return SLIMM_OK;
}

// A window of a file's bytes in one of the eight forms: record bytes (`bytes` are BAM records or SAM text), whole BGZF blocks
// of them (the first `skip` inflated bytes are not records), SAM text in a streamed codec.
int push_window(slimm_ctx* c, const uint8_t* bytes, uint64_t src_bytes, int format, uint32_t skip, int last, uint64_t* n_records) {
    if (!c) return SLIMM_E_INVALID;
    if (n_records) *n_records = 0;
    const Codec codec = format == kFormatBzip2Sam ? Codec::Bzip2 : format == kFormatGzipSam ? Codec::Gzip : format == kFormatZstdSam ? Codec::Zstd : format == kFormatXzSam ? Codec::Xz : format == kFormatLz4Sam ? Codec::Lz4 : format == kFormatLzipSam ? Codec::Lzip : Codec::None;
    const bool sam = format == kFormatSam || format == kFormatBgzfSam || codec != Codec::None;
    Push p{bytes, src_bytes, src_bytes, skip, last != 0, sam, codec, format == kFormatBgzf || format == kFormatBgzfSam};
    SLIMM_TRY(check_push(c, p));
    (void)hipSetDevice(c->device);
    HIP_TRY(c, need_stream(c->copy_stream, kStreamHigh));
    SLIMM_TRY(open_file(c, p));
    WindowPipeline& W = c->win;
    File& F = W.file;
    uint64_t total = 0;
    push_trace("push: %.0f MB %s -> %.0f MB%s", p.src_bytes / 1e6, p.compressed ? "of blocks" : "inflated", p.n_bytes / 1e6, p.last ? " (last)" : "");
    if (p.codec != Codec::None)
        SLIMM_TRY(push_stream(c, p, total));
    else if (p.n_bytes && p.compressed)
        SLIMM_TRY(gather_blocks(c, p, total));
    else if (p.n_bytes || (p.sam && p.last && !W.announced.ends_mid && (F.sam_last_byte != '\n' || F.sam_dev_tail)))
        SLIMM_TRY(push_plain(c, p));
    if (p.last) SLIMM_TRY(launch_gathered(c));
    // ... while the windows before are worked on: the oldest are finished -- all of them when this is the file's end
    const bool had_any = F.head < F.windows;
    SLIMM_TRY(finish_windows(c, p.last ? Upto::All : Upto::Lag, p.last, true, total));
    if (p.last) {
        if (!had_any && F.carry_bytes && !W.announced.ends_mid) return fail(c, SLIMM_E_INVALID, "truncated BAM record");
        F.closed = true;
        W.free_outgrown();
    } else {
        SLIMM_TRY(release_callers_buffer(c, p));
        push_trace("push returns");
    }
    if (n_records) *n_records = total;
    return SLIMM_OK;
}

}  // namespace

extern "C" {

// A caller's host buffer page-locked for the life of the context: the DMA engine then reads it directly (slimm_push_bam_bytes
// and the *_async pushes take any host memory, at the speed of the runtime's own staging when it is pageable)
int slimm_pin_host_buffer(slimm_ctx* c, const void* p, uint64_t n_bytes) {
    if (!c || !p || !n_bytes) return SLIMM_E_INVALID;
    if (c->device < 0) return fail(c, SLIMM_E_INVALID, "host-only context");
    (void)hipSetDevice(c->device);
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (auto& r : c->win.registered)
        if (b >= r.first && b + n_bytes <= r.first + r.second) return SLIMM_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipHostRegister(const_cast<uint8_t*>(b), n_bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, SLIMM_E_HIP, "hipHostRegister failed");
    }
    push_trace("page-locked %.0f MB in %.2f ms", n_bytes / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    c->win.registered.emplace_back(b, static_cast<size_t>(n_bytes));
    return SLIMM_OK;
}

int slimm_set_input_mid_file(slimm_ctx* c, int starts_mid_file, int ends_mid_file) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_input_mid_file: before the range's first window");
    c->win.announced.starts_mid = starts_mid_file != 0;
    c->win.announced.ends_mid = ends_mid_file != 0;
    return SLIMM_OK;
}
int slimm_set_input_range(slimm_ctx* c, uint64_t begin, uint64_t end) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_input_range: before the range's first window");
    if (begin > end) return fail(c, SLIMM_E_INVALID, "slimm_set_input_range: a range ends at or behind its start");
    c->win.announced.has_range = true;
    c->win.announced.range_begin = begin;
    c->win.announced.range_end = end;
    return SLIMM_OK;
}
int slimm_set_gzip_range(slimm_ctx* c, uint64_t begin_bit, uint64_t end_bit) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_gzip_range: before the range's first window");
    if (begin_bit > end_bit) return fail(c, SLIMM_E_INVALID, "slimm_set_gzip_range: a range ends at or behind its start");
    c->win.announced.gz_range = true;
    c->win.announced.gz_begin_bit = begin_bit;
    c->win.announced.gz_end_bit = end_bit;
    return SLIMM_OK;
}
int slimm_set_gzip_window_pass(slimm_ctx* c, int on) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_gzip_window_pass: before the range's first window");
    if (on && !c->win.announced.gz_range) return fail(c, SLIMM_E_INVALID, "slimm_set_gzip_window_pass: slimm_set_gzip_range first");
    c->win.announced.gz_window_pass = on != 0;
    return SLIMM_OK;
}
int slimm_set_xz_range_check(slimm_ctx* c, int check) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_xz_range_check: before the range's first window");
    if (check < -1 || check > 15) return fail(c, SLIMM_E_INVALID, "slimm_set_xz_range_check: a check kind is 0 to 15, or -1 for none told");
    c->win.announced.xz_check = check;
    return SLIMM_OK;
}
int slimm_set_input_size_hint(slimm_ctx* c, uint64_t compressed_bytes) {
    if (!c) return SLIMM_E_INVALID;
    if (c->win.file.active) return fail(c, SLIMM_E_INVALID, "slimm_set_input_size_hint: before the file's first window");
    c->win.announced.size_hint = compressed_bytes;
    return SLIMM_OK;
}
int slimm_window_memory(slimm_ctx* c, uint64_t* device_bytes) {
    if (!c || !device_bytes) return SLIMM_E_INVALID;
    *device_bytes = c->win.held_bytes();
    return SLIMM_OK;
}
int slimm_device_memory(slimm_ctx* c, uint64_t* used_bytes, uint64_t* total_bytes) {
    if (!c || !used_bytes || !total_bytes) return SLIMM_E_INVALID;
    if (c->device < 0) return fail(c, SLIMM_E_INVALID, "host-only context");
    (void)hipSetDevice(c->device);
    size_t fr = 0, tot = 0;
    HIP_TRY(c, hipMemGetInfo(&fr, &tot));
    *used_bytes = tot - fr;
    *total_bytes = tot;
    return SLIMM_OK;
}
int slimm_push_bam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatBam, 0u, last, n_records);
}
int slimm_push_bgzf_blocks(slimm_ctx* c, const uint8_t* blocks, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, blocks, n_bytes, kFormatBgzf, skip, last, n_records);
}
int slimm_push_sam_bytes(slimm_ctx* c, const uint8_t* text, uint64_t n_bytes, int last, uint64_t* n_records) {
    return push_window(c, text, n_bytes, kFormatSam, 0u, last, n_records);
}
int slimm_push_bgzf_sam_blocks(slimm_ctx* c, const uint8_t* blocks, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, blocks, n_bytes, kFormatBgzfSam, skip, last, n_records);
}
int slimm_push_bzip2_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatBzip2Sam, skip, last, n_records);
}
int slimm_push_gzip_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatGzipSam, skip, last, n_records);
}
int slimm_push_zstd_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatZstdSam, skip, last, n_records);
}
int slimm_push_xz_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatXzSam, skip, last, n_records);
}
int slimm_get_xz_stats(slimm_ctx* c, uint64_t out[17]) {
    if (!c || !out) return SLIMM_E_INVALID;
    static_assert(WindowPipeline::kXzStats == 17, "slimm_get_xz_stats: seventeen counters");
    std::copy(c->win.xz_stats, c->win.xz_stats + WindowPipeline::kXzStats, out);
    return SLIMM_OK;
}
int slimm_push_lz4_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatLz4Sam, skip, last, n_records);
}
int slimm_get_lz4_stats(slimm_ctx* c, uint64_t out[16]) {
    if (!c || !out) return SLIMM_E_INVALID;
    static_assert(WindowPipeline::kLzStats == 16, "slimm_get_lz4_stats: sixteen words");
    std::copy(c->win.lz_stats, c->win.lz_stats + WindowPipeline::kLzStats, out);
    return SLIMM_OK;
}
int slimm_push_lzip_sam_bytes(slimm_ctx* c, const uint8_t* bytes, uint64_t n_bytes, uint32_t skip, int last, uint64_t* n_records) {
    return push_window(c, bytes, n_bytes, kFormatLzipSam, skip, last, n_records);
}
int slimm_get_lzip_stats(slimm_ctx* c, uint64_t out[9]) {
    if (!c || !out) return SLIMM_E_INVALID;
    static_assert(WindowPipeline::kLzipStats == 9, "slimm_get_lzip_stats: nine counters");
    std::copy(c->win.lzip_stats, c->win.lzip_stats + WindowPipeline::kLzipStats, out);
    return SLIMM_OK;
}
int slimm_get_zstd_stats(slimm_ctx* c, uint64_t out[20]) {
    if (!c || !out) return SLIMM_E_INVALID;
    static_assert(WindowPipeline::kZsStats == 20, "slimm_get_zstd_stats: twenty counters");
    std::copy(c->win.zs_stats, c->win.zs_stats + WindowPipeline::kZsStats, out);
    return SLIMM_OK;
}
int slimm_get_gzip_stats(slimm_ctx* c, uint64_t out[12]) {
    if (!c || !out) return SLIMM_E_INVALID;
    static_assert(WindowPipeline::kGzStats == 12, "slimm_get_gzip_stats: twelve counters");
    std::copy(c->win.gz_stats, c->win.gz_stats + WindowPipeline::kGzStats, out);
    return SLIMM_OK;
}
// The header's reference names (@SQ SN, index = the reference id) for the SAM pushes: a hash table on the device.
int slimm_set_reference_names(slimm_ctx* c, const char* const* names) {
    if (!c || !names) return SLIMM_E_INVALID;
    if (c->device < 0) return fail(c, SLIMM_E_INVALID, "host-only context has no record stream");
    (void)hipSetDevice(c->device);
    WindowPipeline& W = c->win;
    uint32_t cap = 16;
    while (cap < 2u * c->R + 2u) cap <<= 1;
    std::vector<SamRefEntry> tab(cap);
    for (auto& e : tab) {
        e.hash = 0;
        e.ref = -1;
        e.name_off = e.name_len = e.pad = 0;
    }
    std::vector<uint8_t> blob;
    for (uint32_t r = 0; r < c->R; ++r) {
        const char* nm = names[r] ? names[r] : "";
        const size_t n = strlen(nm);
        const uint64_t h = sam_name_hash(nm, n);
        bool dup = false;
        uint32_t slot = static_cast<uint32_t>(h) & (cap - 1u);
        for (;; slot = (slot + 1u) & (cap - 1u)) {
            if (tab[slot].ref < 0) break;
            if (tab[slot].hash == h && tab[slot].name_len == n && memcmp(blob.data() + tab[slot].name_off, nm, n) == 0) {
                dup = true;   // (two header lines with one name: the first one's index, like the host reader's map)
                break;
            }
        }
        if (dup) continue;
        tab[slot].hash = h;
        tab[slot].ref = static_cast<int32_t>(r);
        tab[slot].name_off = static_cast<uint32_t>(blob.size());
        tab[slot].name_len = static_cast<uint32_t>(n);
        blob.insert(blob.end(), nm, nm + n);
    }
    blob.resize(blob.size() + 16, 0);
    HIP_TRY(c, W.sam_table.ensure(cap));
    HIP_TRY(c, W.sam_names.ensure(blob.size()));
    HIP_TRY(c, hipMemcpy(W.sam_table.p, tab.data(), cap * sizeof(SamRefEntry), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(W.sam_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    W.sam_mask = cap - 1u;
    return SLIMM_OK;
}

}  // extern "C"

namespace slimm {

const StreamCodec& codec_of(WindowPipeline::File::Codec k) { return kCodecs[static_cast<size_t>(k)]; }

int stream_upload(slimm_ctx* c, DevBuf<uint8_t>& comp, uint64_t tail) {
    const std::vector<uint8_t>& pend = c->win.file.stream.pend;
    const uint64_t n = pend.size();
    if (comp.cap < n + tail) HIP_TRY(c, comp.ensure_later(n + (n >> 3) + tail, c->win.outgrown));
    if (n) HIP_TRY(c, hipMemcpyAsync(comp.p, pend.data(), n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(comp.p + n, 0, tail, c->stream));
    return SLIMM_OK;
}

int stream_candidates(slimm_ctx* c, DevBuf<unsigned long long>& d_cand, DevBuf<uint32_t>& count, uint32_t cap, const std::function<void(uint32_t)>& launch,
                      uint32_t* got) {
    for (;; cap = *got + (*got >> 2) + 256u) {   // (more than room: again, with room)
        if (d_cand.cap < cap) HIP_TRY(c, d_cand.ensure_later(cap, c->win.outgrown));
        HIP_TRY(c, hipMemsetAsync(count.p, 0, 4, c->stream));
        launch(cap);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(got, count.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (*got <= cap) return SLIMM_OK;
    }
}

int fetch_filter_stats(slimm_ctx* c, uint64_t* out) {
    WindowPipeline& W = c->win;
    std::fill(out, out + SLIMM_RF_N_STATS, 0ull);
    if (c->device < 0 || !W.file.filter_counted || !W.filter_counts.p) return SLIMM_OK;
    (void)hipSetDevice(c->device);
    uint32_t w[SLIMM_RF_N_STATS] = {};
    HIP_TRY(c, hipMemcpyAsync(w, W.filter_counts.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::copy(w, w + SLIMM_RF_N_STATS, out);
    return SLIMM_OK;
}

int fetch_q18(slimm_ctx* c) {
    WindowPipeline& W = c->win;
    if (!W.carry.p) return SLIMM_OK;
    (void)hipSetDevice(c->device);
    uint32_t w[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(w, &W.carry.p->short_starts, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    W.file.q18_starts = w[0];
    W.file.q18_plain = w[1];
    return SLIMM_OK;
}

// slimm_group_stitch_ranges (split.hip): the head of the member on the right -- n bytes at src, on device src_device -- as one
// more window of this member, behind the incomplete record (SAM: line) its last window ended with.  final: the window must
// end with a complete record; anything else means the right member guessed its first record wrong (SLIMM_E_SPLIT).
// end_line: the window is one newline instead of the head
int append_window(slimm_ctx* c, const uint8_t* src, int src_device, uint64_t n, bool final, uint64_t& n_rec, bool end_line) {
    WindowPipeline& W = c->win;
    File& F = W.file;
    n_rec = 0;
    if (!F.active || !F.closed || F.head != F.windows) return fail(c, SLIMM_E_INVALID, "a range's bytes are joined once it is pushed");
    (void)hipSetDevice(c->device);
    SLIMM_TRY(window_buffer(c, std::max<uint64_t>(n, 1u)));
    const uint64_t j = F.windows;
    uint8_t* dst = W.bytes[next_buffer(F)].p + kBamSlack;
    if (end_line) {   // (SAM: the newline of a last line that lacks one, when the file's last range held no byte to end it)
        n = 1;
        HIP_TRY(c, hipMemsetAsync(dst, '\n', 1, c->stream));
    } else if (n && src_device == c->device) HIP_TRY(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream));
    else if (n)
        HIP_TRY(c, hipMemcpyPeerAsync(dst, c->device, src, src_device, n, c->stream));
    SLIMM_TRY(submit_window(c, n, c->stream, false, n != 0));   // (no bytes: nothing to wait for)
    const bool starts_mid = W.announced.starts_mid;
    W.announced.starts_mid = starts_mid && F.found_start;   // (a range of no record start: its first record is in this window)
    const int rc = finish_window(c, j, n, false, n_rec);
    W.announced.starts_mid = starts_mid;
    ++F.head;
    if (rc != SLIMM_OK) return fail(c, SLIMM_E_SPLIT, "the bytes around a cut: %s", c->err.c_str());
    if (final && F.carry_bytes)
        return fail(c, SLIMM_E_SPLIT, F.sam ? "the line across a cut does not end where the next range's first line starts"
                                            : "the record chain across a cut does not end where the next range's first record was guessed");
    return SLIMM_OK;
}

}  // namespace slimm
