"""Directed zstd inputs, written in plain Python and deterministic: a compressed-block writer with a chosen literals section
(raw and RLE in every size format, Huffman with direct and with FSE-compressed weights, 1 and 4 streams, treeless), a chosen
sequence list (literal length, match length, offset value with the repeat codes) and a chosen mode per table (predefined, RLE,
described, repeat), over an FSE encoder that walks the decoding table backwards.  tests/sam_zst.py's frame_header / block and
XXH64 wrap the blocks.  Every input decodes to a SAM text: its header, `@CO` lines that carry what SAM fields cannot (skipped
with the header), and a few records.  INPUTS() lists them, one path family each, with the paths of tests/zstd_paths.py each is
named for.  Written from RFC 8878; test infrastructure only."""
import heapq
import random
import struct

from tests import sam_zst as Z
from tests.lzma_directed import greedy
from tests.zstd_paths import LL_BASE, LL_BITS, LL_DEFAULT, ML_BASE, ML_BITS, ML_DEFAULT, OF_DEFAULT, fse_table

DEFAULTS = {"ll": LL_DEFAULT, "of": OF_DEFAULT, "ml": ML_DEFAULT}
PREDEFINED, RLE, FSE, REPEAT = 0, 1, 2, 3


def backward(reads) -> bytes:
    """The bitstream a decoder reads as `reads` [(value, bits)], first read first, from the padding mark down."""
    bits = "1" + "".join(format(v, f"0{n}b") for v, n in reads if n)
    return int(bits, 2).to_bytes((len(bits) + 7) // 8, "little")


def fse_description(counts, log) -> bytes:
    """The description of normalised `counts` (-1: less than 1) that add up to 1 << log."""
    out, nbits = log - 5, 4

    def put(v, n):
        nonlocal out, nbits
        out |= v << nbits
        nbits += n

    remaining, i = 1 << log, 0
    while remaining > 0:
        c = counts[i]
        x = c + 1
        bits = (remaining + 1).bit_length()
        lower, threshold = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        if x < threshold:
            put(x, bits - 1)
        elif x <= lower:
            put(x, bits)
        else:
            put(x + threshold, bits)
        remaining -= 1 if c < 0 else c
        i += 1
        if c == 0:
            z = 0
            while counts[i] == 0:
                z, i = z + 1, i + 1
            while z >= 3:
                put(3, 2)
                z -= 3
            put(z, 2)
    assert remaining == 0 and not any(counts[i:]), counts
    return out.to_bytes((nbits + 7) // 8, "little")


def normalised(symbols, log, less_than_1=()):
    """Counts for the histogram of `symbols` that add up to 1 << log, every symbol present with at least 1 (-1 for those of
    `less_than_1`)."""
    hist = {}
    for s in symbols:
        hist[s] = hist.get(s, 0) + 1
    size, total = 1 << log, len(symbols)
    counts = [0] * (max(hist) + 1)
    for s, n in hist.items():
        counts[s] = -1 if s in less_than_1 else max(1, n * size // total)
    rest = size - sum(abs(c) for c in counts)
    order = sorted((s for s in hist if counts[s] > 0), key=lambda s: -counts[s])
    assert order, "every symbol less than 1"
    k = 0
    while rest < 0:      # (take from the largest that can spare one)
        s = order[k % len(order)]
        if counts[s] > 1:
            counts[s] -= 1
            rest += 1
        k += 1
        assert k < 1 << 20, "too many symbols for the accuracy log"
    counts[order[0]] += rest
    return counts


def fse_chain(table, symbols):
    """(the state to start from, [(value, bits)] of the transitions in decoding order) for one state's symbols."""
    by = {}
    for x, (s, nb, base) in enumerate(table):
        by.setdefault(s, []).append((x, nb, base))
    x = max(by[symbols[-1]], key=lambda e: e[1])[0]     # (the last state: one that asks for bits, so that a stream can end on it)
    steps = []
    for s in reversed(symbols[:-1]):
        for cand, nb, base in by[s]:
            if base <= x < base + (1 << nb):
                steps.append((x - base, nb))
                x = cand
                break
        else:
            raise AssertionError("no state")
    return x, steps[::-1]


def code_of(base, v):
    c = max(k for k, b in enumerate(base) if b <= v)
    return c, v - base[c]


# ---- Huffman
def code_lengths(data: bytes, limit=11):
    """{symbol: bits} of a Huffman code for `data`'s bytes, at most `limit` bits."""
    hist = {}
    for c in data:
        hist[c] = hist.get(c, 0) + 1
    assert len(hist) >= 2
    shift = 0
    while True:
        heap = [(max(1, n >> shift), s, (s,)) for s, n in hist.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(hist, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            return depth
        shift += 1


class Huffman:
    def __init__(self, lengths: dict):
        self.max_bits = max(lengths.values())
        assert sum(1 << (self.max_bits - n) for n in lengths.values()) == 1 << self.max_bits and self.max_bits <= 11, lengths
        self.weights = [0] * (max(lengths) + 1)
        for s, n in lengths.items():
            self.weights[s] = self.max_bits + 1 - n
        self.code, at = {}, 0
        for w in range(1, self.max_bits + 1):
            for s, x in enumerate(self.weights):
                if x == w:
                    self.code[s] = (at >> (w - 1), self.max_bits + 1 - w)
                    at += 1 << (w - 1)

    def description(self, how: str) -> bytes:
        """how: "direct", or "fse5" / "fse6" (FSE-compressed weights at that accuracy log)."""
        w = self.weights[:-1]      # (the last symbol's weight follows from the others)
        if how == "direct":
            assert 1 <= len(w) <= 128
            w2 = w + [0]
            return bytes([127 + len(w)]) + bytes((w2[i] << 4) | w2[i + 1] for i in range(0, len(w), 2))
        assert len(w) >= 2
        log = int(how[3:] or 6)
        counts = normalised(w, log)
        table = fse_table(counts, log)
        (x1, t1), (x2, t2) = fse_chain(table, w[0::2]), fse_chain(table, w[1::2])
        reads = [(x1, log), (x2, log)]
        for i in range(len(w) - 2):
            reads.append((t1 if i % 2 == 0 else t2)[i // 2])
        body = fse_description(counts, log) + backward(reads)
        assert len(body) < 128
        return bytes([len(body)]) + body

    def stream(self, data: bytes) -> bytes:
        return backward([self.code[c] for c in data])


# ---- the frame writer
def new(offset: int) -> int:
    """The offset value of a new offset."""
    return offset + 3


REP1, REP2, REP3 = 1, 2, 3
PROBE = [(b"x", 3, REP3), (b"y", 3, REP3), (b"z", 3, REP3)]     # (reads the three repeat offsets back, the last one first; leaves them as they were)


class Frame:
    """One frame, block by block; `out` grows with it.  A sequence is (literals, match length, offset value): REP1 .. REP3 or
    new(offset).  valid=False: for the invalid variants, offsets are not checked against the text."""
    def __init__(self, window_log=17, checksum=True, content_size=False, valid=True):
        self.window_log, self.checksum, self.content_size, self.valid = window_log, checksum, content_size, valid
        self.out, self.reps, self.parts, self.huf, self.tables = bytearray(), [1, 4, 8], [], None, {}

    def raw(self, data: bytes):
        self.parts.append((0, bytes(data), None))
        self.out += data
        return self

    def rle(self, byte: bytes, n: int):
        self.parts.append((1, byte, n))
        self.out += byte * n
        return self

    def _literals(self, lits: bytes, lit):
        kind, fmt = lit[0], lit[1]
        t = ("raw", "rle", "huffman", "treeless").index(kind)
        n = len(lits)
        if t < 2:
            assert n < (32, 4096, 32, 1 << 20)[fmt] and (t == 0 or (n and lits == lits[:1] * n))
            hb = (1, 2, 1, 3)[fmt]
            head = (t | (fmt << 2) | (n << (3 if hb == 1 else 4))).to_bytes(hb, "little")
            return head + (lits if t == 0 else lits[:1])
        if t == 2:
            self.huf = Huffman(lit[3] if len(lit) > 3 and lit[3] else code_lengths(lits))
            desc = self.huf.description(lit[2])
        else:
            desc = b""
            self.huf = self.huf or Huffman(code_lengths(lits))    # (no tree in front: an invalid variant)
        if fmt == 0:
            body = self.huf.stream(lits)
        else:
            each = (n + 3) // 4
            s = [self.huf.stream(lits[k * each:(k + 1) * each]) for k in range(4)]
            body = struct.pack("<3H", len(s[0]), len(s[1]), len(s[2])) + b"".join(s)
        comp, nb, hb = len(desc) + len(body), (10, 10, 14, 18)[fmt], (3, 3, 4, 5)[fmt]
        assert n < 1 << nb and comp < 1 << nb, (n, comp)
        return (t | (fmt << 2) | (n << 4) | (comp << (4 + nb))).to_bytes(hb, "little") + desc + body

    def compressed(self, seqs, tail=b"", lit=("raw", 3), modes=(PREDEFINED, PREDEFINED, PREDEFINED), logs=(6, 5, 6), less_than_1=((), (), ()),
                   tables=None):
        """A compressed block.  modes, logs, less_than_1: per table (literal lengths, offsets, match lengths); tables: counts to
        describe instead of the sequences' own histogram {name: counts}."""
        lits = b"".join(s[0] for s in seqs) + tail
        payload = self._literals(lits, lit)
        n = len(seqs)
        if n == 0:
            payload += b"\x00"
        else:
            payload += bytes([n]) if n < 128 else bytes([128 + (n >> 8), n & 0xff]) if n < 0x7F00 else b"\xff" + struct.pack("<H", n - 0x7F00)
            codes = {"ll": [], "of": [], "ml": []}
            extra = []
            for lit_bytes, ml, ofv in seqs:
                lc, le = code_of(LL_BASE, len(lit_bytes))
                mc, me = code_of(ML_BASE, ml)
                oc = ofv.bit_length() - 1
                codes["ll"].append(lc), codes["of"].append(oc), codes["ml"].append(mc)
                extra.append(((ofv - (1 << oc), oc), (me, ML_BITS[mc]), (le, LL_BITS[lc])))
            payload += bytes([(modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)])
            use = {}
            for k, name in enumerate(("ll", "of", "ml")):
                mode = modes[k]
                if mode == PREDEFINED:
                    self.tables[name] = (fse_table(*DEFAULTS[name]), DEFAULTS[name][1])
                elif mode == RLE:
                    assert len(set(codes[name])) == 1
                    self.tables[name] = ([(codes[name][0], 0, 0)], 0)
                    payload += bytes([codes[name][0]])
                elif mode == FSE:
                    counts = (tables or {}).get(name) or normalised(codes[name], logs[k], less_than_1[k])
                    self.tables[name] = (fse_table(counts, logs[k]), logs[k])
                    payload += fse_description(counts, logs[k])
                else:
                    assert self.valid is False or name in self.tables
                use[name] = self.tables.get(name) or (fse_table(*DEFAULTS[name]), DEFAULTS[name][1])
            chains = {name: fse_chain(use[name][0], codes[name]) for name in use}
            reads = [(chains[name][0], use[name][1]) for name in ("ll", "of", "ml")]
            for i in range(n):
                reads += extra[i]
                if i + 1 < n:
                    reads += [chains["ll"][1][i], chains["ml"][1][i], chains["of"][1][i]]
            payload += backward(reads)
        assert len(payload) <= 1 << 17
        # the text
        out, reps = self.out, self.reps
        for lit_bytes, ml, ofv in seqs:
            out += lit_bytes
            if ofv > 3:
                reps = [ofv - 3] + reps[:2]
            else:
                idx = ofv - 1 + (len(lit_bytes) == 0)
                if idx == 1:
                    reps = [reps[1], reps[0], reps[2]]
                elif idx == 2:
                    reps = [reps[2], reps[0], reps[1]]
                elif idx == 3:
                    reps = [reps[0] - 1, reps[0], reps[1]]
            off = reps[0]
            if self.valid:
                assert 1 <= off <= len(out) and off <= 1 << self.window_log, (off, len(out))
            if off < 1 or off > len(out):
                out += bytes(ml)
                continue
            for _ in range(ml):
                out.append(out[len(out) - off])
        out += tail
        self.reps = reps
        self.parts.append((2, payload, None))
        return self

    def bytes(self, wrong_size=None) -> bytes:
        text = bytes(self.out)
        out = [Z.frame_header(len(text) if self.content_size else None, self.checksum, self.window_log)]
        for i, (kind, payload, n) in enumerate(self.parts):
            out.append(Z.block(kind, payload, n, last=i == len(self.parts) - 1))
        if self.checksum:
            out.append(struct.pack("<I", Z.xxh64(text) & 0xffffffff))
        return b"".join(out)


def sequences_of(history: bytes, data: bytes, window: int):
    """(sequences, tail) of a greedy parse of `data` behind `history`: new offsets only."""
    seqs, lits = [], b""
    for op in greedy(history, data, window, min_len=4, max_len=200):
        if op[0] == "lit":
            lits += op[1]
        else:
            seqs.append((lits, op[2], new(op[1])))
            lits = b""
    return seqs, lits


NAMES = ("literals_raw_rle", "literals_huffman", "table_modes", "mode_bytes", "fse_descriptions", "n_seq_0", "n_seq_127", "n_seq_128", "n_seq_32511",
         "n_seq_32512", "codes_and_extra_bits", "first_sequence_repeats", "repeat_offsets", "repeat_offsets_across_blocks",
         "repeat_offsets_across_frames", "matches_into_earlier_blocks", "checksum_none")
HISTORY = ("repeat_offsets_across_blocks", "matches_into_earlier_blocks")      # (pushed with a round a block too: their force key)


# ---- the inputs -----------------------------------------------------------------------------------------------------------
def _letters(n: int, seed: int, alphabet=b"ACGTNacgtn !#0123456789:;<=>?IJKLMNOPQRST~") -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _line(payload: bytes) -> bytes:
    return b"@CO\t" + payload + b"\n"


def INPUTS(header: bytes, records: bytes):
    """{name: (zstd bytes, text, skip, [paths it is named for], the force key by which a history case is pushed once more, a round a
    block, or None)}."""
    out = {}

    def add(name, frames, paths, force=None, skip=None):
        frames = frames if isinstance(frames, list) else [frames]
        text = b"".join(bytes(f.out) for f in frames)
        out[name] = (b"".join(f.bytes() for f in frames), text, skip if skip is not None else text.index(records), paths, force)

    def start(**kw):
        f = Frame(**kw)
        f.raw(header)
        return f

    def finish(f, **kw):
        """The records as one compressed block of a greedy parse."""
        assert f.out.endswith(b"\n")
        step = 1 << min(f.window_log, 16)      # (a block holds at most the window)
        for i in range(0, len(records), step):
            seqs, tail = sequences_of(bytes(f.out[-(1 << 15):]), records[i:i + step], 1 << min(f.window_log, 15))
            f.compressed(seqs, tail, **({"lit": ("huffman", 1 if step < 4000 else 2, "fse")} | kw))
        return f

    # -- raw and RLE literals in every size format
    f = start()
    for kind in ("raw", "rle"):
        for fmt, n in ((0, 20), (1, 700), (2, 25), (3, 5000)):
            body = _letters(n, fmt) if kind == "raw" else b"r" * n
            lits = b"@CO\t" + body if kind == "raw" else body
            if kind == "rle":
                f.raw(b"@CO\t")
            f.compressed([(lits[:len(lits) // 2], 5, new(3))], lits[len(lits) // 2:], lit=(kind, fmt))
            f.raw(b"\n")
    add("literals_raw_rle", finish(f), [f"lit:{k}:sf{fmt}:streams1" for k in ("raw", "rle") for fmt in range(4)])
    # -- Huffman literals: direct and FSE-compressed weights, 1 and 4 streams in every size format, treeless, 11-bit codes
    f = start()
    for k, (fmt, n, how) in enumerate(((0, 300, "direct"), (1, 900, "fse5"), (2, 3000, "direct"), (3, 9000, "fse6"))):
        lits = _line(_letters(n, 10 + k, b"ACGTNacgtn0123456789 !#:;<=>?"[:8 + 7 * k]))
        f.compressed([(lits[:7], 4, new(2))], lits[7:], lit=("huffman", fmt, how))
        lits = _line(_letters(n // 2, 20 + k, b"ACGTNacgtn0123456789 !#:;<=>?"[:8 + 7 * k]) + b"@CO\t\n")
        f.compressed([(lits[:7], 4, new(2))], lits[7:], lit=("treeless", fmt))
    lengths = {c: min(k + 1, 11) for k, c in enumerate(b"ACGTNacgtn\n@")}       # (1, 2, ... 10, 11, 11 bits)
    lits = b"@" + b"".join(bytes([c]) * (1 << (11 - n)) for c, n in lengths.items() if c not in b"\n@") + b"\n"
    f.compressed([(lits[:9], 6, new(4))], lits[9:], lit=("huffman", 2, "direct", lengths))
    add("literals_huffman", finish(f, lit=("huffman", 2, "direct")),
        [f"lit:huffman:sf{k}:streams{1 if k == 0 else 4}" for k in range(4)] + [f"lit:treeless:sf{k}:streams{1 if k == 0 else 4}" for k in range(4)]
        + ["huf:direct", "huf:fse", "huf:maxbits:11", "fse:weights:al5", "fse:weights:al6"])
    # -- every mode for every table; repeat after predefined, after RLE and after described; RLE tables with many sequences
    f = start()
    word = _letters(40, 30)
    f.raw(b"@CO\t" + word)

    def same(n, k):   # (n sequences of one literal length, offset code and match length each: what RLE tables can carry)
        return [(_letters(2, 100 * k + i), 5, new(9)) for i in range(n)]

    def mixed(n, k):
        return [(_letters(1 + i % 5, 100 * k + i), 4 + i % 7, new(3 + i % 30)) for i in range(n)]

    k = 0
    for first in (PREDEFINED, RLE, FSE):
        for name_at in range(3):
            modes = [PREDEFINED] * 3
            modes[name_at] = first
            f.compressed(same(40, k) if first == RLE else mixed(40, k), modes=tuple(modes))
            modes[name_at] = REPEAT
            f.compressed(same(30, k + 1) if first == RLE else mixed(40, k + 1), modes=tuple(modes))
            k += 2
    f.compressed(same(200, k), modes=(RLE, RLE, RLE))
    f.compressed(same(100, k + 1), modes=(REPEAT, REPEAT, REPEAT))
    f.compressed(mixed(120, k + 2), modes=(FSE, FSE, FSE), logs=(9, 8, 9))
    f.compressed(mixed(60, k + 3), modes=(REPEAT, REPEAT, REPEAT))
    f.raw(b"\n")
    add("table_modes", finish(f, modes=(FSE, FSE, FSE), logs=(7, 6, 7)),
        [f"mode:{t}:{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")]
        + [f"mode:{t}:repeat:after_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse")]
        + [f"mode:{t}:rle:many_sequences" for t in ("ll", "of", "ml")] + ["fse:ll:al9", "fse:of:al8", "fse:ml:al9"])
    # -- all 64 mode bytes: every block can repeat what the block in front set, whatever that was
    f = start()
    f.raw(b"@CO\t" + _letters(20, 33))
    f.compressed(same(5, 900), modes=(FSE, FSE, FSE))
    for m in range(64):
        f.compressed(same(5, 901 + m), modes=(m >> 4, (m >> 2) & 3, m & 3))
    f.raw(b"\n")
    add("mode_bytes", finish(f), [f"mode_byte:0x{m << 2:02x}" for m in range(64)])
    # -- FSE descriptions: probabilities of less than 1, chains of zero-repeat flags, the smallest accuracy log
    f = start()
    f.raw(b"@CO\t" + _letters(70, 40))
    seqs = [(_letters(ll, 41 + i), ml, new(of)) for i, (ll, ml, of) in enumerate([(0, 3, 5), (1, 3, 5), (0, 30, 5), (1, 3, 253), (0, 3, 5), (35, 3, 5), (0, 48, 5)] * 6)]
    f.compressed(seqs, modes=(FSE, FSE, FSE), logs=(5, 5, 5), less_than_1=((22,), (8,), (37,)))
    for log in range(6, 10):      # (every accuracy log a table may have)
        f.compressed([(_letters(1 + i % 5, 400 + i), 4 + i % 7, new(3 + i % 30)) for i in range(60)], modes=(FSE, FSE, FSE), logs=(log, min(log, 8), log))
    f.raw(b"\n")
    add("fse_descriptions", finish(f), [f"fse:{t}:{p}" for t in ("ll", "of", "ml") for p in ("less_than_1", "zero_repeat_chain")]
        + [f"fse:{t}:al{k}" for t, top in (("ll", 9), ("of", 8), ("ml", 9)) for k in range(5, top + 1)])
    # -- the sequence count's forms
    for n in (0, 127, 128, 0x7EFF, 0x7F00):
        f = start()
        f.raw(b"@CO\tab")
        if n:
            f.compressed([(b"", 3, new(2))] * n, b"\n", modes=(RLE, RLE, RLE))
        else:
            f.compressed([], b"no sequences\n")
        add(f"n_seq_{n}", finish(f), [f"nseq:{n}", {0: "nseq:0", 127: "nseq:1byte", 128: "nseq:2byte", 0x7EFF: "nseq:2byte", 0x7F00: "nseq:3byte"}[n]])
    # -- every code with its extra bits all zeros and all ones: offset codes up to the window's, literal lengths, match lengths
    f = start(window_log=21, checksum=True)      # (2 MiB: with the xz far-distance input the text of all inputs stays under 8 MiB)
    f.raw(b"@CO\t")
    filler = _letters(4093, 50, b"ACGTacgt0123456789")
    while len(f.out) < (1 << 21):
        f.raw((filler * 33)[:min(1 << 17, (1 << 21) - len(f.out))])
    seqs = []
    for oc in range(2, 22):
        seqs += [(b"o", 3, 1 << oc)] + ([(b"O", 3, (2 << oc) - 1)] if oc < 21 else [])
    seqs += [(b"w", 3, new(1 << 21)), (b"r", 3, REP1), (b"r", 3, REP2), (b"r", 3, REP3)]
    f.compressed(seqs, modes=(RLE, FSE, RLE), logs=(5, 6, 5))
    seqs, k = [], 0
    for c in range(53):     # (a block regenerates at most 128 KiB: match length code 52 cannot have all its extra bits set)
        for ml in sorted({ML_BASE[c], min(ML_BASE[c] + (1 << ML_BITS[c]) - 1, (1 << 17) - 1)}):
            seqs.append((b"m", ml, new(7)))
            if sum(m + 1 for _, m, _ in seqs) > 50_000 or c == 52:
                one = len({m for _, m, _ in seqs}) == 1
                f.compressed(seqs, modes=(RLE, RLE, RLE if one else FSE if k % 2 else PREDEFINED), logs=(5, 5, 6))
                seqs, k = [], k + 1
    for c in range(36):     # (... and literal length code 35 neither, with a match behind it)
        for n in sorted({LL_BASE[c], min(LL_BASE[c] + (1 << LL_BITS[c]) - 1, (1 << 17) - 3)}):
            big = n >= 64          # (as RLE literals, so that the block's own bytes stay under its maximum)
            f.compressed([(b"l" * n if big else _letters(n, c), 3, new(7))], lit=("rle" if big else "raw", 3), modes=(PREDEFINED if c % 2 else RLE, RLE, RLE))
    f.raw(b"\n")
    add("codes_and_extra_bits", finish(f), [f"of_code:{c}" for c in range(22)] + [f"ll_code:{c}" for c in range(36)] + [f"ml_code:{c}" for c in range(53)]
        + [f"of_code:{c}:{e}" for c in range(2, 21) for e in ("zeros", "ones")] + [f"ll_code:{c}:{e}" for c in range(16, 35) for e in ("zeros", "ones")]
        + [f"ml_code:{c}:{e}" for c in range(32, 52) for e in ("zeros", "ones")] + ["ll_code:35:zeros", "ml_code:52:zeros", "of_code:21:zeros", "reach:window_edge"])
    # -- repeat offsets: the first sequence of a frame against the start values 1 / 4 / 8
    frames = []
    for k, (ofv, ll) in enumerate(((REP1, 9), (REP2, 9), (REP3, 9), (REP1, 0), (REP2, 0))):
        f = Frame()
        if k == 0:
            head = header
        else:
            head = b"@CO\t" + _letters(5, 60 + k)
        if ll:
            f.compressed([(head, 6, ofv), (b"x", 3, REP2), (b"", 3, REP1)] + PROBE, b"\n" if k else b"")
        else:   # (no literals in front: the text comes from a raw block, which leaves the offsets alone)
            f.raw(head)
            f.compressed([(b"", 6, ofv), (b"x", 3, REP2), (b"", 3, REP1)] + PROBE, b"\n")
        if k == 0:
            f.raw(b"@CO\tthe first frame\n")
        frames.append(f)
    frames.append(finish(Frame().raw(b"@CO\n")))
    add("first_sequence_repeats", frames, [f"of:rep:first_of_frame:idx{i}" for i in range(3)])
    # -- rep1 - 1 with no literals in front, on a plain offset and on an entry offset, twice in a row; 3, 2, 1, 0 entry slots alive
    f = start()
    f.raw(b"@CO\t" + _letters(100, 70))
    f.compressed([(b"a", 4, new(40)), (b"", 4, REP3), (b"", 4, REP3), (b"bc", 3, new(50)), (b"d", 3, new(60))] + PROBE)       # (plain: 40 -> 39 -> 38)
    f.compressed([(b"", 4, REP3), (b"", 4, REP3), (b"e", 3, REP1)] + PROBE)                   # (entry slot 0: 60 -> 59 -> 58; slots 1 and 2 behind it)
    f.compressed([(b"f", 4, REP1)] + PROBE)                                                   # (3 alive)
    f.compressed([(b"g", 4, REP2), (b"", 4, REP1), (b"", 4, REP2)] + PROBE)                   # (3 alive, turned round)
    f.compressed([(b"h", 4, new(33))] + PROBE)                                                # (2 alive)
    f.compressed([(b"i", 4, new(34)), (b"j", 4, new(35))] + PROBE)                            # (1 alive)
    f.compressed([(b"k", 4, new(36)), (b"l", 4, new(37)), (b"m", 4, new(38))] + PROBE)        # (0 alive)
    f.compressed([(b"n", 4, REP3), (b"", 4, REP3), (b"o", 3, REP2), (b"", 5, REP2)] + PROBE)
    f.compressed([(b"p", 4, new(41)), (b"q", 4, new(51)), (b"r", 3, new(61))])
    f.compressed([(b"s", 4, REP2), (b"", 4, REP3), (b"t", 3, REP1)] + PROBE)                  # (entry slot 1, 51, to the front; 50; 50 again)
    f.compressed([(b"u", 4, REP3), (b"", 4, REP3), (b"v", 3, REP1)] + PROBE, b"\n")           # (entry slot 2 likewise)
    add("repeat_offsets", finish(f), ["of:rep:idx3:plain", "of:rep:idx3:entry", "of:rep:entry_slot0:decremented1", "of:rep:idx1:ll0", "of:rep:idx2:ll0",
                                      "of:rep:idx1:ll>0", "of:rep:idx2:ll>0", "of:rep:entry_slot0:decremented2", "of:rep:entry_slot1:decremented1",
                                      "of:rep:entry_slot2:decremented1"] + [f"exit:entry_slots_alive:{n}" for n in range(4)])
    # -- the same chains across a raw block, an RLE block, a compressed block without sequences; and across rounds
    for name, force in (("repeat_offsets_across_blocks", "zstd_round_text=1,zstd_round=1"),):
        f = start()
        f.raw(b"@CO\t" + _letters(100, 80))
        f.compressed([(b"a", 4, new(40)), (b"b", 4, new(50)), (b"c", 3, new(60))])
        for between in ("raw", "rle", "none", "compressed"):
            if between == "raw":
                f.raw(_letters(9, 81))
            elif between == "rle":
                f.rle(b"=", 9)
            elif between == "none":
                f.compressed([], _letters(9, 82))
            f.compressed([(b"", 4, REP3), (b"", 4, REP3), (b"e", 3, REP2), (b"", 5, REP1), (b"f", 5, REP3)] + PROBE)
        f.raw(b"\n")
        add(name, finish(f), ["reps:carried_over_raw_block", "reps:carried_over_rle_block", "reps:carried_over_compressed_block_without_sequences",
                              "reps:carried_into_compressed_block", "of:rep:entry_slot0:decremented1"], force)
    # -- ... and across a frame boundary, where they start again
    f = start()
    f.raw(b"@CO\t" + _letters(100, 90))
    f.compressed([(b"a", 4, new(40)), (b"b", 4, new(50)), (b"c", 3, new(60))], b"\n")
    g = Frame()
    g.rle(b"@", 1).raw(b"CO\t" + _letters(20, 91))
    g.compressed([(b"", 4, REP2), (b"", 4, REP3), (b"e", 3, REP2), (b"", 5, REP1)] + PROBE, b"\n")      # (8, not 40: then 7, 8, 7)
    add("repeat_offsets_across_frames", [f, finish(g)], ["of:rep:first_of_frame:idx2", "of:rep:idx3:entry", "block:first:rle"])
    # -- matches into each kind of earlier block, and to the window's exact edge at windowLog 10
    for name, force in (("matches_into_earlier_blocks", "zstd_round_text=1,zstd_round=1"),):
        f = Frame(window_log=10)
        f.raw(header[:len(header) // 2])
        f.raw(header[len(header) // 2:] + b"@CO\t")
        f.rle(b"-", 300)
        f.compressed([(b"ab", 5, new(100)), (b"c", 5, new(788))], _letters(300, 95))             # (into the RLE block; to the frame's first byte, in the raw one)
        f.compressed([(b"d", 5, new(200)), (b"e", 9, new(1024))])                                # (into the compressed one; the window's edge)
        f.raw(_letters(1024 - 15, 96))
        f.compressed([(b"", 15, new(1024))], b"\n")
        add(name, finish(f), [f"reach:earlier_block:{k}" for k in ("raw", "rle", "compressed")] + ["reach:window_edge", "reach:frame_start"], force)
    # -- the no-checksum path only
    f = start(checksum=False)
    f.compressed([(b"@CO\t" + _letters(30, 97), 9, new(11))], b"\n")
    add("checksum_none", finish(f), [])
    assert tuple(out) == NAMES, list(out)
    return out


def INVALID(header: bytes, records: bytes):
    """{name: (zstd bytes, the decoder's words)}: what a decoder must refuse, each one rule broken in an otherwise good frame."""
    out = {}

    def start(**kw):
        f = Frame(valid=False, **kw)
        f.raw(header + b"@CO\t" + _letters(50, 1))
        return f

    f = start()
    f.compressed([(b"", 4, REP3)], b"\n")             # (the start value 1, minus 1)
    out["rep1_minus_1_is_zero"] = (f.bytes(), "an offset beyond the frame's start or window")
    f = start()
    f.compressed([(b"a", 4, new(len(f.out) + 2))], b"\n")
    out["offset_one_beyond_the_frames_start"] = (f.bytes(), "an offset beyond the frame's start or window")
    f = start(window_log=10)
    f.raw(_letters(550, 2)).raw(_letters(550, 3))
    f.compressed([(b"a", 4, new(1025))], b"\n")
    out["offset_one_beyond_the_window"] = (f.bytes(), "an offset beyond the frame's start or window")
    for k, name in enumerate(("literal_lengths", "offsets", "match_lengths")):
        f = start()
        modes = [PREDEFINED] * 3
        modes[k] = REPEAT
        f.compressed([(b"a", 4, new(5))], b"\n", modes=tuple(modes))
        out[f"repeat_mode_with_nothing_to_repeat_{name}"] = (f.bytes(), "a repeated table with none in front to repeat")
    f = start()
    f.compressed([(b"a", 4, new(5))], b"\n", lit=("treeless", 0))
    out["treeless_literals_with_no_tree"] = (f.bytes(), "a repeated table with none in front to repeat")
    return out
