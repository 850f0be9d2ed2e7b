// lzip-compressed SAM decoded on the device (include/slimm_hip.h: slimm_push_lzip_sam_bytes; the format: lzip_member.h, the
// member finder: lzip_walk.h).  A file is members back to back -- `plzip` writes one per block of twice its dictionary size --,
// each a raw LZMA stream with an empty dictionary and fresh state in front of it, and every member's trailer states its own
// size, its text's size and its text's CRC32: the host finds every whole member at hand without decoding a bit, and knows the
// exact place of its text before a kernel runs.  The bytes at hand go through stages, a ROUND:
//   (host)          lzip::Walker names the whole members at hand; the text offsets are a prefix sum of the stated data_sizes
//   k_lzip_decode   a workgroup of one wave per member, the probabilities in LDS: all lanes set them, the FIRST lane decodes
//                   the stream (lzip::lzma_member: xz_stream.h's decoder, ended by the marker) straight to the member's place
//                   in the round's text -- which is its dictionary: a match copies from the member's own earlier output
//   k_xz_check, k_xz_fold (xz_decode.hip: launch_xz_checks)   the member's CRC32 over pieces of text, folded per member
//   (host)          the registers against the trailers' CRC32 fields
// No workgroup waits for another.  One round is one window; the window then goes to the SAM finder and decoder as any text
// window does (windows.hip).  An lzip stream is not cut by byte range.  NOT MEASURED on an MI355X: nothing is known of an LZMA
// lane's rate there.
#include "context.h"
#include "split_plan.h"
#include "host/lzip.cpp"   // (lzip_read_index, for slimm_host_lzip_members: the library holds no other copy of it)

namespace slimm {
namespace {

constexpr uint64_t kLzipTail = 16;                      // zeroed bytes behind the compressed bytes on the device
constexpr uint64_t kLzipRoundText = 512ull << 20;       // a round's text at most (SLIMM_FORCE lzip_round_text=N), or one member alone
constexpr uint64_t kLzipMemberTextMax = 1ull << 30;     // one member of more text than that is refused, as an xz block is
using LF = WindowPipeline::File::Lzip;

// (a decoder is ONE lane of a wave of its own, as k_xz_decode's: lanes of one wave that decode different members would take
// each other's branches in turn.  lc + lp = 3 always, so the probabilities are 15 980 bytes: ten such workgroups share a CU's
// 160 KiB of LDS, where k_xz_decode's 28 268 bytes -- sized for lc + lp = 4 -- let five)
__global__ __launch_bounds__(64) void k_lzip_decode(const uint8_t* __restrict__ comp, uint64_t n_bytes, xz::Block* __restrict__ members, uint32_t n,
                                                     uint8_t* __restrict__ text, uint64_t text_cap) {
    __shared__ uint16_t probs[lzip::kProbs];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    for (uint32_t k = lane; k < lzip::kProbs; k += 64u) probs[k] = xz::kProbInit;
    __syncthreads();
    if (lane != 0) return;
    xz::Block& b = members[i];
    const uint64_t at = b.at, end = b.end, text_at = b.text_at, text_len = b.text_len;
    xz::Tally tally{0, 0};
    uint32_t st = lzip::kOverrun;
    // (the stream lies in the bytes, the text in the buffer: no read and no write outside either, whatever the stream says)
    if (at < end && end <= n_bytes && text_len <= kLzipMemberTextMax && text_at <= text_cap && text_len <= text_cap - text_at)
        st = lzip::lzma_member(comp, at, end, probs, text + text_at, static_cast<uint32_t>(text_len), b.dict_size, tally);
    b.status = st;
    b.match_bytes = tally.match_bytes;
    b.max_dist = tally.max_dist;
}

void push_trace_lzip(const char* fmt, ...) {   // "[push lzip] ..."
    va_list ap;
    va_start(ap, fmt);
    push_trace_line("lzip", fmt, ap);
    va_end(ap);
}

// the host reader's words (host/alignment_file.cpp: codec_read)
int lzip_fail(slimm_ctx* c, const std::string& where, uint32_t status) {
    return fail(c, SLIMM_E_INVALID, "lzip-compressed input is not supported unless it decodes: %s: %s", where.c_str(), lzip::status_text(status));
}

}  // namespace

bool lzip_next_window(const slimm_ctx* c, uint64_t, uint64_t* n) {   // (a round's text is one window: kLzipRoundText)
    const LF& Z = c->win.file.lzip;
    *n = Z.text - std::min(Z.text, c->win.file.stream.skip_left);
    return !Z.ready.empty();
}

int lzip_round(slimm_ctx* c, bool last) {
    WindowPipeline& W = c->win;
    LF& Z = W.file.lzip;
    WindowPipeline::File::Stream& T = W.file.stream;
    Z.ready.clear(), Z.ready_at.clear();
    Z.text = 0;
    if (T.waiting && !last) return SLIMM_OK;
    T.waiting = false;   // (at the file's end what waited for bytes is looked at again: it is the last member, or is truncated)
    // (errors come in file order: what is wrong behind members that are ready is looked at again by the next round, once those
    // members are decoded -- RoundCursor::hold)
    RoundCursor cur(c, W, last, "lzip", "member", "member");
    const uint64_t cap_text = forced_or("lzip_round_text", kLzipRoundText, 1);
    using Walk = lzip::Walker;
    Walk& K = Z.walk;
    uint64_t text = 0;
    uint32_t pieces = 0;
    for (;;) {
        const Walk::Item it = K.peek(cur.p(), cur.avail(), cur.at(), last);
        if (it.kind == Walk::MayEnd) {   // (the file may end here)
            cur.wait();
            break;
        }
        if (it.kind == Walk::More) {   // (a member whose end is not at hand waits for the next push; the search keeps its place)
            K.take(it);
            SLIMM_TRY(cur.wait_or(it.where(), it.words()));
            break;
        }
        if (it.kind == Walk::Error) {
            SLIMM_TRY(cur.fail_words(it.words()));
            break;
        }
        const uint64_t mtext = it.trailer.data_size, stream = it.bytes - lzip::kHeaderBytes - lzip::kTrailerBytes;
        if (mtext > kLzipMemberTextMax && lzip::text_fits_stream(mtext, stream)) {
            if (!cur.hold) return fail(c, SLIMM_E_INVALID, "an lzip member of more than 1 GiB of text: decode this file on the host");
            break;
        }
        if (!lzip::text_fits_stream(mtext, stream)) {   // (the host reader's verdict on such a data_size)
            SLIMM_TRY(cur.fail_words(it.where() + ": " + lzip::status_text(lzip::kMarkerEarly)));
            break;
        }
        if (!Z.ready.empty() && text + mtext > cap_text) break;   // (the round is full: this member starts the next one)
        K.take(it);
        xz::Block b{};
        b.at = cur.pos + lzip::kHeaderBytes, b.end = b.check_at = cur.pos + it.bytes - lzip::kTrailerBytes;
        b.text_at = text, b.text_len = mtext;
        b.dict_size = it.dict_size, b.check = xz::kCheckCrc32, b.piece0 = pieces, b.status = lzip::kOk;
        const uint64_t tail = mtext % gz::kPiece ? mtext % gz::kPiece : (mtext ? gz::kPiece : 0u);
        b.last_mul = gz::crc_x_pow8(tail);
        pieces += static_cast<uint32_t>((mtext + gz::kPiece - 1u) / gz::kPiece);
        Z.ready.push_back(b);
        Z.ready_at.push_back(it.at);
        cur.hold = true;
        text += mtext;
        cur.pos += it.bytes;
    }
    Z.text = text;
    return SLIMM_OK;
}

int lzip_emit(slimm_ctx* c, uint8_t* dst, uint64_t, uint64_t* n_out, uint8_t* last_byte) {
    WindowPipeline& W = c->win;
    LF& Z = W.file.lzip;
    WindowPipeline::Lzip& S = W.lzs;
    hipStream_t st = c->stream;
    uint64_t* stats = W.lzip_stats;
    const uint32_t nm = static_cast<uint32_t>(Z.ready.size());
    const uint64_t text = Z.text;
    *n_out = 0;
    if (!nm) return SLIMM_OK;
    const uint64_t drop = W.file.stream.skip_of(text);
    const uint32_t pieces = Z.ready.back().piece0 + static_cast<uint32_t>((Z.ready.back().text_len + gz::kPiece - 1u) / gz::kPiece);
    if (S.text.cap < text + 1u) HIP_TRY(c, S.text.ensure_later(text + (text >> 3) + 1u, W.outgrown));
    if (S.members.cap < nm) HIP_TRY(c, S.members.ensure_later(nm + (nm >> 2) + 64u, W.outgrown));
    if (S.piece.cap < pieces + 1u) HIP_TRY(c, S.piece.ensure_later(pieces + (pieces >> 3) + 1u, W.outgrown));
    SLIMM_TRY(stream_upload(c, S.comp, kLzipTail));
    HIP_TRY(c, hipMemcpyAsync(S.members.p, Z.ready.data(), nm * sizeof(xz::Block), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lzip_decode, dim3(nm), dim3(64), 0, st, S.comp.p, W.file.stream.pend.size(), S.members.p, nm, S.text.p, text);
    launch_xz_checks(st, S.members.p, nm, pieces, S.text.p, S.piece.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Z.ready.data(), S.members.p, nm * sizeof(xz::Block), hipMemcpyDeviceToHost, st));
    if (text > drop) {
        HIP_TRY(c, hipMemcpyAsync(dst, S.text.p + drop, text - drop, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(last_byte, dst + (text - drop) - 1u, 1, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    ++stats[WindowPipeline::kLzipRounds];
    const uint8_t* p = W.file.stream.pend.data();
    for (uint32_t k = 0; k < nm; ++k) {
        const xz::Block& b = Z.ready[k];
        const std::string where = lzip::place_text(Z.ready_at[k]);
        if (b.status != lzip::kOk) return lzip_fail(c, where, b.status);
        const uint32_t reg = gz::crc_mul(0xffffffffu, gz::crc_x_pow8(b.text_len)) ^ static_cast<uint32_t>(b.crc);
        if (xz::le32(p + b.check_at) != ~reg) return lzip_fail(c, where, lzip::kBadCrc);
        ++stats[WindowPipeline::kLzipMembers];
        ++stats[WindowPipeline::kLzipCrc32];
        if (!b.text_len) ++stats[WindowPipeline::kLzipEmpty];
        stats[WindowPipeline::kLzipMatchBytes] += b.match_bytes;
        stats[WindowPipeline::kLzipMaxDist] = std::max<uint64_t>(stats[WindowPipeline::kLzipMaxDist], b.max_dist);
        stats[WindowPipeline::kLzipMaxDict] = std::max<uint64_t>(stats[WindowPipeline::kLzipMaxDict], b.dict_size);
    }
    stats[WindowPipeline::kLzipText] += text;
    *n_out = text - drop;
    push_trace_lzip("round %llu: %u members -> %.1f MB of text", (unsigned long long)stats[WindowPipeline::kLzipRounds], nm, text / 1e6);
    Z.ready.clear();
    Z.text = 0;
    return SLIMM_OK;
}

void lzip_trace_file(const slimm_ctx* c) {
    if (!traced("push")) return;
    const uint64_t* s = c->win.lzip_stats;
    fprintf(stderr, "[push lzip] %llu members (%llu empty) in %llu rounds; %llu CRC32 checked; %llu match bytes, longest distance %llu, largest "
                    "dictionary %llu; %llu compressed bytes -> %llu bytes of text\n",
            (unsigned long long)s[WindowPipeline::kLzipMembers], (unsigned long long)s[WindowPipeline::kLzipEmpty], (unsigned long long)s[WindowPipeline::kLzipRounds],
            (unsigned long long)s[WindowPipeline::kLzipCrc32], (unsigned long long)s[WindowPipeline::kLzipMatchBytes], (unsigned long long)s[WindowPipeline::kLzipMaxDist],
            (unsigned long long)s[WindowPipeline::kLzipMaxDict], (unsigned long long)s[WindowPipeline::kLzipCompressedBytes], (unsigned long long)s[WindowPipeline::kLzipText]);
}

}  // namespace slimm

extern "C" {

// The members of an lzip file by its trailers, from the file's end (host/lzip.cpp: lzip_read_index): a few reads, nothing decoded
int slimm_host_lzip_members(const char* path, uint64_t* n_members, uint64_t* text_bytes) {
    slimm::PlanFile f;
    std::vector<slimm::LzipIndexMember> members;
    if (!path || !n_members || !text_bytes || !f.open_regular(path) || !slimm::lzip_read_index(f.reader(), f.size, &members)) return SLIMM_E_INVALID;
    *n_members = members.size();
    *text_bytes = 0;
    for (const slimm::LzipIndexMember& m : members) *text_bytes += m.data_size;
    return SLIMM_OK;
}

}  // extern "C"
