// The window pipeline's state (windows.hip; the streamed codecs' decoders and split.hip work on it too), in three parts by how long they
// live: what the context keeps (buffers, streams, events), what the caller announces for the next file, and the file's own
// state, which is reset in one place.  Included by context.h (DevBuf, PinBuf).
#pragma once

struct slimm_ctx;
namespace slimm {

struct WindowPipeline {
    // The ring of window buffers [slack | window]: a window is copied -- or inflated -- into one while older ones are still
    // on their way or being decoded: at most kWindowLag of them, and at most kWindowInFlight bytes; the incomplete record at
    // a window's end is copied in front of the next window.  Windows that arrive as BGZF blocks are gathered into device
    // windows of up to kWindowGather inflated bytes, three of which keep both inflate streams busy; a ring of 16 buffers of
    // that size was 20 - 25 GB of HBM per context, ADVICE round 4
    static constexpr uint32_t kWindowRing = 4, kWindowLag = kWindowRing - 2;
    static constexpr uint64_t kWindowInFlight = 4ull << 30;    // finish the oldest window when more than this is in flight
    static constexpr uint64_t kWindowGather = 1900ull << 20;   // inflated bytes of a gathered device window (a window is < 2 GiB)
    static constexpr uint64_t kWindowGatherGoal = 1400ull << 20;  // ... which is launched once it holds this much
    static constexpr uint64_t kWindowKeepAcrossFiles = 4ull << 30; // end_file gives the pipeline's buffers back above this

    // ---- as long as the context
    DevBuf<uint8_t> bytes[kWindowRing];
    DevBuf<BamPiece> pieces;
    DevBuf<uint32_t> offs;
    DevBuf<BamCarry> carry;
    PinBuf<BamWindowResult> result;     // written by k_bam_scan straight into page-locked host memory
    std::vector<std::pair<const uint8_t*, size_t>> registered;  // caller buffers page-locked by hipHostRegister
    hipEvent_t copied[kWindowRing] = {};   // the window's bytes are in its buffer (behind the copy, or behind the inflate)
    hipEvent_t h2d_done[4] = {};        // the caller's buffer of a push has been read (the pushes' events, in turn)
    // windows that arrive as BGZF blocks (slimm_push_bgzf_blocks, slimm_push_bgzf_sam_blocks): compressed bytes + block
    // descriptors per buffer, the inflater's scratch and {error code, first bad block, -, last line ended} per buffer
    DevBuf<uint8_t> comp[kWindowRing];
    DevBuf<BgzfBlock> desc[kWindowRing];
    std::vector<BgzfBlock> desc_host[kWindowRing];   // (a buffer's descriptors stay until the buffer's turn comes again: the copy reads them)
    DevBuf<uint8_t> inflate_scratch[2];
    DevBuf<uint32_t> inflate_status;       // 4 words per buffer
    PinBuf<uint32_t> h_inflate_status;     // ... fetched with the window's other results
    // the inflate kernels' own streams, taken in turn by the device windows: the copies of other windows go on beside
    // them, and the Huffman phase of one window (a lane per block: 30 K blocks are half the lanes) beside the other's
    hipStream_t inflate_stream[2] = {nullptr, nullptr};
    hipEvent_t comp_copied = nullptr;
    std::vector<void*> outgrown;   // device buffers replaced by larger ones while kernels were in flight: freed at the file's end
    // SAM text (sam_decode.hip): the header's reference names as a hash table on the device (slimm_set_reference_names)
    DevBuf<SamRefEntry> sam_table;
    DevBuf<uint8_t> sam_names;
    uint32_t sam_mask = 0;
    // a byte range of a split file (split.hip): the head, the first record's name, the left member's carry, the guess
    DevBuf<uint8_t> head_bytes;
    DevBuf<BamCarry> first, join;
    DevBuf<unsigned long long> guess;
    // the record filter (record_filter.h; slimm_set_record_filter): part of the configuration -- it outlives a file -- and
    // the decoders' counters of the file at hand (SLIMM_RF_N_STATS words, zeroed by open_file when the filter is on)
    slimm_record_filter filter{};
    DevBuf<uint32_t> filter_counts;
    // bzip2 SAM (bzip2_decode.hip), the decode scratch: the compressed bytes not decoded yet, the candidates (block magics),
    // and per slot of a batch the BWT string -- then its RLE1 text --, the inverse BWT's links, the byte histogram, what
    // decoding found and the text's length
    struct Bzip2 {
        DevBuf<uint8_t> comp, ll;
        DevBuf<uint32_t> link, hist, count, text_len;
        DevBuf<unsigned long long> d_cand;
        DevBuf<bz2::BlockInfo> info;
        DevBuf<int64_t> out_at;
        template <typename F>
        void each_held(F&& f) { f(comp), f(ll), f(link), f(hist), f(d_cand); }   // (the large ones: see each_held below)
        uint64_t held() {
            uint64_t n = 0;
            each_held([&](auto& b) { n += b.cap * sizeof(*b.p); });
            return n;
        }
    } bz2;
    // gzip SAM (gzip_decode.hip), the decode scratch: the compressed bytes not decoded yet, the block candidates and chunk
    // starts, the size pass's results, the chain's chunks, the round's text as 16-bit symbols (a byte, or a marker for a
    // byte of the chunk in front), the chunks' last 32 768 bytes (slot 0: those of the round before), the pieces' CRCs
    struct Gzip {
        DevBuf<uint8_t> comp, win;
        DevBuf<unsigned long long> d_cand;
        DevBuf<uint32_t> count, flag;
        DevBuf<gz::Walk> walk;
        DevBuf<gz::Chunk> chunks;
        DevBuf<uint16_t> sym;
        DevBuf<uint2> piece;
        // a byte range of a split file: the window pass's 16-bit windows (slot k as win's: a byte, or a marker into the
        // 32 768 bytes in front of the RANGE), and the 32 768 bytes in front of the range that the member on the left
        // installed for the text pass (slimm_group_gzip_windows; 64 KiB: not counted, not given back between the passes)
        DevBuf<uint16_t> win16;
        DevBuf<uint8_t> front, applied;
        template <typename F>
        void each_held(F&& f) { f(comp), f(win), f(d_cand), f(flag), f(walk), f(chunks), f(sym), f(piece), f(win16); }
    } gz;
    // gzip SAM by byte range, what a member keeps between its window pass and its text pass (slimm_group_gzip_windows), and
    // the text pass must reproduce: where its chain ended (the file's bit) and its text's length
    struct GzipPass {
        bool done = false;        // the window pass ran to its last push
        bool has_front = false;   // gz.front holds the bytes in front of the range, front_len of them valid
        uint32_t front_len = 0;
        uint64_t end_bit = 0, text = 0;
    } gz_pass;
    // the counters of the gzip file read last (slimm_get_gzip_stats): they outlive the file's state
    enum { kGzMembers, kGzChunks, kGzCandidates, kGzDropped, kGzStored, kGzFixed, kGzDynamic, kGzResolved, kGzRounds, kGzText, kGzCompressed, kGzForced, kGzStats };
    uint64_t gz_stats[kGzStats] = {};

    // zstd SAM (zstd_decode.hip), the decode scratch: the compressed bytes of a round and what its blocks repeat of the
    // blocks in front, the blocks' descriptors, the decoded literals and sequences, the round's text behind its history
    // (the frame's last window of text), the position each text byte copies from, the history kept for the next round
    struct Zstd {
        DevBuf<uint8_t> comp, lit, text, hist;
        DevBuf<zs::Block> blocks;
        DevBuf<zs::Seq> seq;
        DevBuf<uint32_t> src;
        PinBuf<uint8_t> h_text;             // the round's text on the host, for the content checksums (released by end_file)
        DevBuf<unsigned long long> count;   // [0] passes' "changed", [1] bad offsets, [2] first block with one, [3], [4]: stats 13, 14
        template <typename F>
        void each_held(F&& f) { f(comp), f(lit), f(text), f(hist), f(blocks), f(seq), f(src); }
    } zst;
    // the counters of the zstd file read last (slimm_get_zstd_stats): they outlive the file's state
    enum { kZsFrames, kZsSkippable, kZsRaw, kZsRle, kZsCompressed, kZsHufTree, kZsTreeless, kZsLitPlain, kZsPredefined, kZsRleTable, kZsFseTable,
           kZsRepeated, kZsSequences, kZsFromFront, kZsFromHistory, kZsRounds, kZsText, kZsCompressedBytes, kZsChecksums, kZsPasses, kZsStats };
    uint64_t zs_stats[kZsStats] = {};

    // lz4 SAM (lz4_decode.hip), the decode scratch: the compressed bytes of a round, the blocks' descriptors and sequences, the
    // round's text behind its history (a linked frame's last 64 KiB), the position each text byte copies from, the history
    // kept for the next round
    struct Lz4 {
        DevBuf<uint8_t> comp, text, hist;
        DevBuf<lz4::Block> blocks;
        DevBuf<lz4::Seq> seq;
        DevBuf<uint32_t> src;
        PinBuf<uint8_t> h_text;             // the round's text on the host, for the content checksums (released by end_file)
        DevBuf<unsigned long long> count;   // as Zstd's: [0] passes' "changed", [1] bad offsets, [2] first block with one, [3], [4]: stats 6, 7
        template <typename F>
        void each_held(F&& f) { f(comp), f(text), f(hist), f(blocks), f(seq), f(src); }
    } lz;
    // the counters of the lz4 file read last (slimm_get_lz4_stats: 16 words, the last two 0): they outlive the file's state
    enum { kLzFrames, kLzSkippable, kLzLinked, kLzStored, kLzCompressed, kLzSequences, kLzFromFront, kLzFromHistory, kLzRounds, kLzText,
           kLzCompressedBytes, kLzBlockSums, kLzContentSums, kLzPasses, kLzStats = 16 };
    uint64_t lz_stats[kLzStats] = {};

    // xz SAM (xz_decode.hip), the decode scratch: the compressed bytes of a round, a descriptor per block, the round's text
    // (which is each block's dictionary as well), the check register of every piece of text (gz::kPiece bytes)
    struct Xz {
        DevBuf<uint8_t> comp, text;
        DevBuf<xz::Block> blocks;
        DevBuf<xz::Piece> piece;
        template <typename F>
        void each_held(F&& f) { f(comp), f(text), f(blocks), f(piece); }
    } xzs;
    // the counters of the xz file read last (slimm_get_xz_stats): they outlive the file's state
    enum { kXzStreams, kXzBlocks, kXzLzmaChunks, kXzRawChunks, kXzStateResets, kXzPropChanges, kXzOddProps, kXzCheckNone, kXzCheckCrc32, kXzCheckCrc64,
           kXzSha256Unverified, kXzMatchBytes, kXzMaxDist, kXzRounds, kXzText, kXzCompressedBytes, kXzIndexRecords, kXzStats };
    uint64_t xz_stats[kXzStats] = {};

    // lzip SAM (lzip_decode.hip), the decode scratch, as Xz's: the compressed bytes of a round, a descriptor per member (an
    // xz::Block whose check is CRC32), the round's text (each member's dictionary as well), the CRC32 register of every piece
    struct Lzip {
        DevBuf<uint8_t> comp, text;
        DevBuf<xz::Block> members;
        DevBuf<xz::Piece> piece;
        template <typename F>
        void each_held(F&& f) { f(comp), f(text), f(members), f(piece); }
    } lzs;
    // the counters of the lzip file read last (slimm_get_lzip_stats): they outlive the file's state
    enum { kLzipMembers, kLzipEmpty, kLzipRounds, kLzipCrc32, kLzipMatchBytes, kLzipMaxDist, kLzipMaxDict, kLzipText, kLzipCompressedBytes, kLzipStats };
    uint64_t lzip_stats[kLzipStats] = {};

    // ---- announced before the file's first window (slimm_set_input_size_hint, slimm_set_input_mid_file), cleared when it ends
    struct Announced {
        uint64_t size_hint = 0;   // the file's compressed bytes (0 = not told): what its gathered windows are sized for
        // a byte range of a file split over a group: it starts inside the file (its first record is guessed; the bytes in
        // front, the head, wait on the device for the member on the left) and / or ends inside it (the carry stays)
        bool starts_mid = false, ends_mid = false;
        // ... and where the range lies in the file (slimm_set_input_range; bzip2 SAM: blocks belong to the range their
        // magic's first bit lies in, and the stitch compares absolute bit positions)
        bool has_range = false;
        uint64_t range_begin = 0, range_end = 0;
        // xz SAM: the check kind of the stream among whose blocks the range starts (slimm_set_xz_range_check; -1: the range
        // starts at a stream header, which tells it)
        int xz_check = -1;
        // gzip SAM: the range in BITS of the file (slimm_set_gzip_range; the member reads the bytes that hold them), and
        // whether the pushes to come are the window pass (slimm_set_gzip_window_pass)
        bool gz_range = false, gz_window_pass = false;
        uint64_t gz_begin_bit = 0, gz_end_bit = 0;
    } announced;

    // ---- this file: reset as a whole, by end_file alone -- a new member needs its initialiser and nothing else
    struct File {
        bool active = false;                // this file's records come through the window pipeline
        bool closed = false;                // the file's last window went in
        bool sam = false;                   // its windows are SAM text
        uint64_t windows = 0;               // handed over so far
        uint64_t head = 0;                  // ... of which [head, windows) are not finished yet (copied / inflating / waiting)
        uint64_t win_bytes[kWindowRing] = {};  // record bytes of the windows in flight
        bool inflated[kWindowRing] = {};    // that window was inflated here
        uint64_t carry_bytes = 0;
        uint64_t pushes = 0;                // pushes that started a copy
        // BGZF pushes gathered for the next device window (buffer windows % kWindowRing): compressed bytes so far, inflated
        // bytes so far, the inflated bytes in front of the file's first record
        bool acc_open = false;
        uint64_t acc_src = 0, acc_dst = 0;
        uint32_t acc_skip = 0, acc_tok = 0;   // (acc_tok: words of token room of the gathered blocks)
        // from the size hint and the first push's ratio: the inflated bytes a gathered window's buffer gets (0 = kWindowGather)
        uint64_t win_cap = 0;
        bool planned = false;               // the file's first COMPRESSED push has reserved its buffers (or found no hint)
        // SAM text: the last byte pushed (a last line without its newline gets one) -- unless the text's last bytes so far
        // were inflated on the device: the device then ends such a line; lines it ended so far (SLIMM_TRACE=push)
        uint8_t sam_last_byte = '\n';
        bool sam_dev_tail = false;
        uint64_t sam_lines_ended = 0;
        // Q18 on a grouped stream (kernels.h: BamCarry): the decoders' two counts of the windows finished so far; a range
        // of a split file: summed by the group (slimm_group_stitch_ranges), not checked per member
        uint64_t q18_starts = 0, q18_plain = 0;
        bool q18_by_group = false;
        bool filter_counted = false;   // filter_counts holds this file's verdicts (the filter was on when the file began)
        bool found_start = false;   // a range that starts inside the file: its first window holds a record start (false: all head)
        bool has_first = false;     // `first` holds the name of the range's first record (decoded in any window)
        uint64_t head_len = 0;
        // a streamed codec's SAM (bzip2, gzip, zstd, xz, lz4, lzip: the file's bytes as they lie in it, decoded here), what every codec
        // keeps on the host: the compressed bytes not decoded yet (file offset `base` on; `bit`: the next bit to read --
        // zstd reads at bytes), the decoded bytes still to skip (the header)
        enum class Codec : uint8_t { None, Bzip2, Gzip, Zstd, Xz, Lz4, Lzip };
        struct Stream {
            Codec codec = Codec::None;
            std::vector<uint8_t> pend;
            uint64_t base = 0, bit = 0;
            uint64_t skip_left = 0;
            bool waiting = false;   // the codec stopped for want of bytes: nothing to decode until pend grows
            // bzip2, gzip: the block candidates found in pend (bit offsets, in order); found: cand holds those of pend as
            // it is, and the device has pend's bytes (zstd sends a round's bytes with every round: never set)
            std::vector<uint64_t> cand;
            bool found = false;
            // What the rounds so far have read goes; the bit to read next stays in the first byte.  Once per round, at its
            // start, and only while the device does not hold pend (windows.hip: push_stream)
            void drop_read() {
                const size_t drop = static_cast<size_t>(bit >> 3);
                pend.erase(pend.begin(), pend.begin() + static_cast<long>(drop));
                base += drop;
                bit -= drop * 8u;
            }
            // the decoded bytes of `text` that are still header: skipped, and counted off
            uint64_t skip_of(uint64_t text) {
                const uint64_t drop = std::min(text, skip_left);
                skip_left -= drop;
                return drop;
            }
        } stream;
        // bzip2 SAM, the host's side: the stream being read (its level, combined CRC so far), the next candidate to look
        // at; the blocks of the last batch decoded and not yet written into a window
        struct Bzip2 {
            bool in_stream = false;
            uint32_t level = 0, combined = 0, streams = 0;
            size_t next_cand = 0;
            uint32_t slots = 0;     // blocks a batch decodes at most (the scratch holds that many; sized per file: bz2_reserve)
            struct Ready {
                uint32_t slot, crc;
                uint64_t len, drop;   // text bytes; of them the first `drop` are skipped (the header)
                uint64_t at;          // file offset of the block (errors)
                bool unchecked = false;   // the first block of a range that starts inside the file: a CRC mismatch is SLIMM_E_SPLIT
            };
            std::vector<Ready> ready;
            size_t ready_pos = 0;
            uint64_t blocks = 0, batches = 0, false_magics = 0;   // (SLIMM_TRACE=push; false_magics: candidates the chain passed over)
            double ms_find = 0, ms_decode = 0, ms_bwt = 0, ms_emit = 0;
            // a byte range of a split file (Announced::has_range).  A range that starts inside the file starts its chain
            // at its first element -- the first block candidate that decodes, or an end-of-stream marker in front of it --
            // inside a stream whose level it does not know: until its first end-of-stream marker it keeps the largest
            // block and the combined CRC from 0 over its blocks (`combined`), which the stitch checks against the chain on
            // its left (bzip2_decode.hip: split_bz2_chains).  A range that ends inside the file stops at the first element that
            // starts at or behind its end.  Bit positions are the file's
            struct Chain {
                bool started = false;        // the chain has its first element (a range from the file's start: its stream header)
                bool ended = false;          // ... and has stopped: at the range's end, or for want of an element of its own
                bool any = false;            // it holds an element of its own
                bool at_file_end = false;    // it stopped behind an end-of-stream marker with no byte left
                uint64_t first_bit = 0, end_bit = 0;
                bool first_stream = false;   // still in the stream the range started in
                uint32_t first_blocks = 0, first_combined = 0, first_max_n = 0;
                uint64_t first_max_at = 0;   // file offset of the largest block of that stream
                bool has_eos = false;        // the range's first stream ended with a marker: its combined CRC, its file offset
                uint32_t eos_crc = 0;
                uint64_t eos_at = 0;
            } chain;
        } bz2;
        // gzip SAM, the host's side: where in a member stream.bit (an exact start) is, the member's CRC register and length
        // so far; the chain's chunks of the round at hand
        struct Gzip {
            enum Stage { Header, Deflate, Trailer } stage = Header;
            uint32_t crc = 0xffffffffu;
            uint64_t len = 0;
            bool carried = false;    // slot 0 of the window scratch holds the last 32 768 bytes of the text so far
            std::vector<gz::Chunk> ready;
            // a byte range of a split file (Announced::gz_range).  A range that starts inside the file starts among a
            // member's blocks: `front` bytes of that member lie in front of it (32 768 assumed until the stitch of the
            // windows knows), crc is a register from 0 and len the range's share (`partial`) until the member's trailer,
            // which it cannot check: what it read there is kept for the stitch (gzip_decode.hip: split_gz_chains)
            bool window_pass = false;   // this file's pushes are the window pass: no text, no CRC
            bool partial = false;
            bool range_done = false;    // the chain stands on the range's end bit
            uint32_t front = 0;
            uint64_t text = 0;          // text bytes of the range so far
            struct LeftTrailer {
                bool has = false;
                uint32_t partial_crc = 0, crc32 = 0, isize = 0;
                uint64_t partial_len = 0, at = 0;   // (at: the trailer's file offset)
            } left;
        } gz;
        // zstd SAM, the host's side: where in the container stream.bit is (zstd_walk.h: the stage, the frame's header and
        // file offset, the frames so far) and what the frame's blocks hand on (the descriptions a block may repeat, the
        // repeat offsets, the text's length and XXH64 so far), the bytes of history the device holds; the blocks and
        // frames of the round at hand
        struct Zstd {
            zs::Walker walk;
            uint64_t frame_len = 0;
            zs::Entropy entropy;
            uint32_t rep[3] = {1, 4, 8};
            zs::Xxh64 xxh{};
            uint64_t hist_len = 0;
            struct Frame {   // a frame with blocks in the round
                uint32_t first = 0, n = 0;   // its blocks of the round
                bool ends = false, has_sum = false;
                uint32_t sum = 0;
                zs::FrameHeader fh{};
                uint64_t at = 0, len_before = 0, text_at = 0, text_len = 0;
                uint32_t rep[3] = {1, 4, 8};   // the repeat offsets and the XXH64 state in front of its blocks of the round
                zs::Xxh64 xxh{};
            };
            std::vector<zs::Block> ready;
            std::vector<uint64_t> ready_at;   // the blocks' file offsets (errors)
            std::vector<Frame> frames;
            std::vector<uint8_t> aux;
            uint64_t text = 0;                // the round's text bytes (behind zs_round)
            uint64_t round_hist = 0;
        } zst;
        // xz SAM, the host's side: where in the container stream.bit is (xz_walk.h: between streams or among a stream's
        // blocks, the stream's check kind and its blocks so far -- what its index must say); the blocks of the round at hand
        struct Xz {
            xz::Walker walk;
            std::vector<xz::Block> ready;
            std::vector<uint64_t> ready_at;   // the blocks' file offsets (errors)
            uint64_t text = 0;                // the round's text bytes (behind xz_round)
            // a byte range of a split file (Announced::has_range).  A range that was told a check kind starts among the
            // blocks of a stream whose header lies on its left (xz::Walker::among_blocks): that stream's index hands back the
            // records in front of the range's own -- the blocks of the ranges on the left --, kept for the stitch (xz_decode.hip:
            // split_xz_streams).  A range that ends among a stream's blocks leaves its blocks of that stream in walk.records
            bool started = false;        // the walk has taken its start from what was announced
            bool from_left = false;      // the range starts among the blocks of a stream
            uint64_t left_index_at = 0;  // ... and has met that stream's index (walk.open_left is off again) at this file offset
            std::vector<xz::Walker::Record> left_kept;
        } xz;
        // lz4 SAM, the host's side: where in the container stream.bit is (lz4_walk.h) and what the frame's blocks hand on (the
        // text's length and XXH32 so far), the bytes of history the device holds; the blocks and frames of the round at hand
        struct Lz4 {
            lz4::Walker walk;
            uint64_t frame_len = 0;
            lz4::Xxh32 xxh{};
            uint64_t hist_len = 0;
            bool in_round = false;   // the frame at hand has blocks in the round: frames.back() is it
            struct Frame {   // a frame with blocks in the round
                uint32_t first = 0, n = 0;   // its blocks of the round
                bool ends = false, has_sum = false;
                uint32_t sum = 0;
                lz4::FrameHeader fh{};
                uint64_t at = 0, len_before = 0, text_at = 0, text_len = 0;
                lz4::Xxh32 xxh{};   // the XXH32 state in front of its blocks of the round
            };
            std::vector<lz4::Block> ready;
            std::vector<uint64_t> ready_at;   // the blocks' file offsets (errors)
            std::vector<Frame> frames;
            uint64_t text = 0;                // the round's text bytes (behind lz4_round)
        } lz;
        // lzip SAM, the host's side: the member finder (lzip_walk.h: the members so far, and how far the member at stream.bit
        // has been searched for its end); the members of the round at hand
        struct Lzip {
            lzip::Walker walk;
            std::vector<xz::Block> ready;
            std::vector<uint64_t> ready_at;   // the members' file offsets (errors)
            uint64_t text = 0;                // the round's text bytes (behind lzip_round)
        } lzip;
    } file;

    // the buffers that grow with a file's windows: what held_bytes() counts is what end_file gives back
    template <typename F>
    void each_held(F&& f) {
        for (uint32_t k = 0; k < kWindowRing; ++k) f(bytes[k]), f(comp[k]), f(desc[k]);
        for (auto& sc : inflate_scratch) f(sc);
        f(pieces), f(offs);
        bz2.each_held(f);
        gz.each_held(f);
        zst.each_held(f);
        xzs.each_held(f);
        lz.each_held(f);
        lzs.each_held(f);
    }
    uint64_t held_bytes() {   // device memory of the window pipeline (slimm_window_memory)
        uint64_t n = 0;
        each_held([&](auto& b) { n += b.cap * sizeof(*b.p); });
        return n;
    }
    void free_outgrown();
    // slimm_reset: abandoned windows and an unlaunched gather waited for, `outgrown` freed, the file's and the announced
    // state fresh, the buffers given back when they hold more than kWindowKeepAcrossFiles.  No HIP call unless windows or a
    // gather are pending or there is something to free (a host-only context is reset too)
    int end_file(slimm_ctx* c);
    // slimm_destroy, once the context's main and copy streams are idle: the inflate streams waited for and destroyed, the
    // caller's buffers unlocked, `outgrown` freed, the events destroyed (the buffers free themselves)
    void destroy();
};

// What the rounds of the codecs that walk a container share (zs_round, xz_round; the walkers: zstd_walk.h, xz_walk.h): the
// byte position in stream.pend, and what a walker's "needs more bytes" or error becomes.  A byte range of a split file
// (check_push: its range is announced) starts and ends at the codec's boundaries or the cut is refused -- SLIMM_E_SPLIT, no
// verdict on the file: the caller reads it through one context.  The range rules, once:
//   an error, or a shortfall at the last push, on the range's FIRST item    the range starts mid-file    no_start
//   a shortfall at the last push                                            the range ends mid-file      no_end
//   anything else                                                                                        the codec's words
int fail(slimm_ctx* c, int code, const char* fmt, ...);
struct RoundCursor {
    slimm_ctx* c;
    WindowPipeline::File::Stream& T;
    const WindowPipeline::Announced& A;
    const char *codec, *start_noun, *end_noun;   // "zstd", "frame", "frame"; "xz", "stream", "block"
    const bool last, starts_mid, ends_mid;
    uint64_t pos;        // the next byte of stream.pend (these codecs read at bytes): put back into stream.bit however the round ends
    bool hold = false;   // blocks in front are ready: an error behind them waits until they are decoded (errors come in file order)
    RoundCursor(slimm_ctx* ctx, WindowPipeline& W, bool last_push, const char* name, const char* starts_at, const char* ends_at)
        : c(ctx), T(W.file.stream), A(W.announced), codec(name), start_noun(starts_at), end_noun(ends_at), last(last_push),
          starts_mid(A.has_range && A.starts_mid), ends_mid(A.has_range && A.ends_mid), pos(T.bit >> 3) {}
    ~RoundCursor() { T.bit = pos * 8u; }
    const uint8_t* p() const { return T.pend.data() + pos; }
    uint64_t avail() const { return T.pend.size() - pos; }
    uint64_t at() const { return T.base + pos; }   // the position as a file offset
    int wait() { return T.waiting = true, SLIMM_OK; }   // more bytes may come
    // the host reader's words (host/alignment_file.cpp: codec_read)
    int fail_words(const std::string& words) {
        return hold ? SLIMM_OK : fail(c, SLIMM_E_INVALID, "%s-compressed input is not supported unless it decodes: %s", codec, words.c_str());
    }
    int no_start(const char* what) {
        return hold ? SLIMM_OK : fail(c, SLIMM_E_SPLIT, "%s: the range starts at byte %llu, where no %s starts", codec, static_cast<unsigned long long>(at()), what);
    }
    int no_end(const std::string& where) {
        return hold ? SLIMM_OK : fail(c, SLIMM_E_SPLIT, "%s: %s runs past byte %llu: the range does not end at a %s boundary", codec, where.c_str(),
                                      static_cast<unsigned long long>(A.range_end), end_noun);
    }
    // what a step lacks: more bytes may come, or the file ends inside it
    int wait_or(const std::string& where, const std::string& words) {
        if (!last) return wait();
        return ends_mid ? no_end(where) : fail_words(words);
    }
    // A walker's outcome that is no item -- an error, or a shortfall (`where`, and `words` with its cause) --, `between`:
    // where a frame / stream may start, `any` of which have been met.  SLIMM_OK: the round ends and waits, or holds
    int settle(bool error, bool between, bool any, const std::string& where, const std::string& words) {
        const bool first = between && starts_mid && !any;
        if (error) return first ? no_start(start_noun) : fail_words(words);
        if (!between) return wait_or(where, words);
        if (!last || (avail() == 0 && (any || starts_mid || ends_mid))) return wait();   // (the file may end here; a range may be empty)
        if (ends_mid) return no_end("what starts at byte " + std::to_string(at()));
        return first ? no_start(start_noun) : fail_words(words);
    }
};

// SLIMM_TRACE=push: what the pipeline does and when, on stderr: "[push <ms since the first line>] ...", or "[push <tag>] ..."
void push_trace_line(const char* tag, const char* fmt, va_list ap);
void push_trace(const char* fmt, ...);
int fetch_filter_stats(slimm_ctx* c, uint64_t* out);   // the filter's counters of the file so far (every window launched); zeros without one
int fetch_q18(slimm_ctx* c);   // the Q18 run counts of the device decoders so far (every window launched) -> file.q18_*
// `n` bytes at `src` (on device src_device) as one more window behind the closed file's carry (split.hip); end_line: one
// newline instead
int append_window(slimm_ctx* c, const uint8_t* src, int src_device, uint64_t n, bool final, uint64_t& n_rec, bool end_line = false);
// What a streamed codec supplies to the pipeline (windows.hip: kCodecs, push_stream), all on file.stream and the codec's own
// state.  round: what can be decoded of stream.pend, up to its text lengths; at `last` what is left must end the streams
// (nothing ready: the bytes wait for more -- stream.waiting --, or the streams have ended).  next_window: is anything
// ready, and *n the text bytes of the next window, at most `cap` where a round's text is cut into several (and at least
// one block).  emit: those written to dst on the context's stream behind what is still to skip of the header (*n_out
// bytes, *last_byte the last of them), their checksums checked.  trace_file: SLIMM_TRACE=push, the file's counters.
//
// bzip2_decode.hip (slimm_push_bzip2_sam_bytes): a round is the next batch of whole blocks, found by their magics and chained
// from the stream header on; a batch's text is cut into windows block by block
int bz2_decode_batch(slimm_ctx* c, bool last);
bool bz2_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int bz2_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
void bz2_trace_file(const slimm_ctx* c);
// (StreamCodec::stitch) the members' block chains against each other, left to right, on host scalars: every chain ends at the
// bit where the next member that holds an element starts, that member's blocks fit the stream's level, and the combined CRC
// of a stream over a cut is its marker's
int split_bz2_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// gzip_decode.hip (slimm_push_gzip_sam_bytes): the member headers and trailers at stream.bit read on the host; then one
// round on the device -- candidates found, chunk starts chosen, the size pass, the chain from the exact start -- which
// leaves the chain's chunks in file.gz.ready.  gz_emit: the chunks decoded, resolved and written behind each other, their
// members' CRC registers and lengths stepped
int gz_round(slimm_ctx* c, bool last);
bool gz_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int gz_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
void gz_trace_file(const slimm_ctx* c);
// split_gz_windows (StreamCodec::window_stitch), between the members' window pass and their text pass, left to right: member
// k's chain ended on member k + 1's first bit; its final 16-bit window, resolved against the bytes in front of its own range
// (launch_gz_window_apply on its device), becomes the 32 768 bytes in front of member k + 1's, copied device to device, with
// how many of them belong to the open gzip member; then every member's file state is fresh for the text pass, its
// announcements kept.  split_gz_chains (StreamCodec::stitch), on host scalars: every chain ended on its range's end and the
// text pass reproduced the window pass's end bit and text length (SLIMM_E_SPLIT), and the CRC register and length of a gzip
// member that lies over cuts, folded left to right, are its trailer's (SLIMM_E_INVALID, the single context's words)
int split_gz_windows(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
int split_gz_chains(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// (a byte range of a split file, between its two passes -- split_gz_windows) out[i] = the byte that the range's
// final 16-bit window win16 names: its own, or byte m of the 32 768 in `front` of the range
void launch_gz_window_apply(hipStream_t st, const uint16_t* win16, const uint8_t* front, uint8_t* out);
// zstd_decode.hip (slimm_push_zstd_sam_bytes): zs_round takes the container's items from zs::Walker (zstd_walk.h) -- the
// format's rules are there, the range rules in RoundCursor above --, plans the whole blocks of stream.pend up to the round's
// text cap, decodes their literals and sequences on the device and leaves the round's blocks, with their text lengths, in
// file.zst.ready.  zs_emit: the text built behind the history, resolved, and written to dst; zs_check, behind the window's
// launch: the content checksums of the frames that ended
// (A byte range of a split file -- Announced::has_range --: the range starts at a frame and ends between frames; nothing in
// front of the range exists for it, and an empty range, or one of skippable frames only, decodes no text)
constexpr uint64_t kZstdRoundBytes = 32ull << 20;   // compressed bytes gathered for a round; also the least a member's range of a split file is worth (slimm_zstd_split_floor)
int zs_round(slimm_ctx* c, bool last);
bool zs_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int zs_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
int zs_check(slimm_ctx* c);
void zs_trace_file(const slimm_ctx* c);
// (StreamCodec::stitch) left to right on host scalars, every member's decoder stands between frames at its range's end with
// every byte of the range read (SLIMM_E_SPLIT otherwise)
int split_zstd_ends(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// The copies of a round's text resolved (lz_resolve.hip; zs_emit, lz4_emit): src[i] is the position in [history H | text] that
// text byte i copies from (itself: a literal, already written).  Pointer doubling until nothing changes -- at most
// ceil(log2(text + H)) + 1 passes, counted into *passes --, then the match bytes fetched from where their chains end.
// count (device, 5 words as Zstd::count) is fetched into `got` behind every pass: got[1] != 0 -- the expand kernel met an
// offset out of reach -- ends it early, for the caller to say in its codec's words
int resolve_copies(slimm_ctx* c, const char* codec, uint32_t* src, uint8_t* text, uint64_t H, uint64_t n_text, unsigned long long* count,
                   unsigned long long got[5], uint32_t* passes);
uint32_t copy_grid_for(uint64_t n);   // the grid of a kernel with a thread per text byte (256 threads a workgroup)
// lz4_decode.hip (slimm_push_lz4_sam_bytes): lz4_round takes the container's items from lz4::Walker (lz4_walk.h), checks the
// block checksums of the whole blocks at hand, has k_lz4_tokens walk their sequences and leaves the round's blocks, with their
// text lengths, in file.lz.ready.  lz4_emit: the text built behind the history, resolved, and written to dst; lz4_check,
// behind the window's launch: the content checksums of the frames that ended.  An lz4 stream is not cut by byte range
constexpr uint64_t kLz4RoundBytes = 32ull << 20;   // compressed bytes gathered for a round: zstd's, a stated default
int lz4_round(slimm_ctx* c, bool last);
bool lz4_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int lz4_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
int lz4_check(slimm_ctx* c);
void lz4_trace_file(const slimm_ctx* c);
// xz_decode.hip (slimm_push_xz_sam_bytes): xz_round takes the container's items from xz::Walker (xz_walk.h), a block's
// chunks up to its end -- a block whose bytes are not all at hand is left at its header --, and leaves the whole blocks at
// hand, with their exact text offsets, in file.xz.ready.  xz_emit: the blocks decoded, a lane each, their checks folded
// from pieces and compared, the text written to dst.
// (A byte range of a split file -- Announced::has_range --: the range starts at a stream header or, told the stream's check
// kind, at a block's first byte, and ends at a block's first byte or between streams; nothing in front of the range exists
// for it, and an empty range decodes no text)
int xz_round(slimm_ctx* c, bool last);
bool xz_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int xz_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
void xz_trace_file(const slimm_ctx* c);
// (StreamCodec::stitch) left to right on host scalars, every member's walker stands at its range's end with every byte of the
// range read; a member that was told a check kind has a stream over the cut in front of it, of that kind; the blocks of such
// a stream in the ranges on the left are, in order and in number, the index records that the member which met the index kept
// (those in front of its own blocks' records)
int split_xz_streams(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
// (xz_decode.hip) k_xz_check and k_xz_fold on a round's blocks -- xz_emit's, and lzip_emit's, whose members are blocks with a
// CRC32 check: every block's register from 0 over its text, into Block::crc
void launch_xz_checks(hipStream_t st, xz::Block* blocks, uint32_t n, uint32_t n_pieces, const uint8_t* text, xz::Piece* piece);
// lzip_decode.hip (slimm_push_lzip_sam_bytes): lzip_round takes the whole members at hand from lzip::Walker (lzip_walk.h) -- a
// member whose end is not at hand waits, the search keeping its place -- and leaves them, with their exact text offsets, in
// file.lzip.ready.  lzip_emit: the members decoded, a lane each, their CRC32 folded from pieces and compared with the
// trailers', the text written to dst.  An lzip stream is not cut by byte range
constexpr uint64_t kLzipRoundBytes = 32ull << 20;   // compressed bytes gathered for a round: xz's, a stated default
int lzip_round(slimm_ctx* c, bool last);
bool lzip_next_window(const slimm_ctx* c, uint64_t cap, uint64_t* n);
int lzip_emit(slimm_ctx* c, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
void lzip_trace_file(const slimm_ctx* c);
// the decoders' shared steps (windows.hip).  stream.pend to the device, into `comp` with `tail` zeroed bytes behind it.
// The candidates a find kernel left at d_cand, counted at count[0]: `launch(cap)` runs it with room for cap of them, again
// with more room when there were more; *got of them are there (and the stream is idle)
int stream_upload(slimm_ctx* c, DevBuf<uint8_t>& comp, uint64_t tail);
int stream_candidates(slimm_ctx* c, DevBuf<unsigned long long>& d_cand, DevBuf<uint32_t>& count, uint32_t cap, const std::function<void(uint32_t)>& launch,
                      uint32_t* got);

// ONE ROW PER STREAMED CODEC (windows.hip: kCodecs, by File::Codec; the row of Codec::None is empty): the hooks above, and the
// codec's side of a file split by byte range over a group's members (split.h).  A new codec is a row and its decoder's file
struct StreamCodec {
    using File = WindowPipeline::File;
    const char* name;        // traces and error texts
    // compressed bytes gathered on the host before a round looks at them (the command's pushes are larger, the ABI's may be
    // of any size); SLIMM_FORCE <round_key>=N: rounds of N bytes -- tests cut blocks, headers and trailers across rounds
    const char* round_key;
    uint64_t round_bytes;
    bool cut_by_range;       // a byte range of a split file may cut it (slimm_set_input_mid_file)
    bool cut_at_frames;      // ... only where the caller's plan found a frame start (xz: a block start): not without slimm_set_input_range
    int (*round)(slimm_ctx*, bool last);
    bool (*next_window)(const slimm_ctx*, uint64_t cap, uint64_t* n);
    int (*emit)(slimm_ctx*, uint8_t* dst, uint64_t cap, uint64_t* n_out, uint8_t* last_byte);
    int (*behind_submit)(slimm_ctx*);   // on the host, beside the window's decode -- also behind a round of no text (or null)
    void (*trace_file)(const slimm_ctx*);
    // where between its streams the codec is: a push's rounds go on while the file offset or this moves, and stop when the
    // codec waits for bytes (null: they go on while a round leaves something ready)
    int (*stage)(const File&);
    bool (*ended)(const File&);   // the codec has stopped for good: bytes pushed now are dropped (or null)
    // its counters (they outlive the file: slimm_get_*_stats), how many, and which of them counts the compressed bytes
    uint64_t* (*stats)(WindowPipeline&);
    size_t n_stats, stat_compressed;
    const char* article;     // "an" where the name wants it (null: "a")
    const char* cut_unit;    // cut_at_frames: what a range starts at (null: "frame")
    // ---- a file split by byte range.  split_range takes a pushed range of this codec only when slimm_set_input_range announced it
    bool range_announced;
    // slimm_group_stitch_ranges, before any text is joined: the members' ranges held against each other, left to right, by the
    // hook of MEMBER 0's codec (null: nothing to hold).  SLIMM_OK, or the code with the message on member *bad: SLIMM_E_SPLIT
    // is wrapped in `stitch_split` (member, message), anything else is member_failed's "<stitch_noun>: <message>".
    // window_stitch: the same between the members' two passes, slimm_group_gzip_windows (null: the codec has one pass)
    int (*stitch)(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
    const char *stitch_split, *stitch_noun;
    int (*window_stitch)(slimm_ctx* const* members, uint32_t n, uint32_t* bad);
};
const StreamCodec& codec_of(WindowPipeline::File::Codec k);

}  // namespace slimm
