"""DEFLATE streams written by hand, bit by bit, from RFC 1951 / RFC 1952: the writers of fixed and dynamic blocks with chosen
code lengths and tokens, the streams zlib would never emit (by class, valid and invalid), gzip framing around them, a writer
that takes a SAM text and a list of tokens checked against it, and the directed inputs of the device's gzip decoder
(slimm_amd/csrc/deflate_stream.h, gzip_decode.hip): a path family each, the crafted block at a chunk start.
tests/deflate_paths.py shows which paths each reaches.  INPUTS(header, body) -> {name: (blob, text, skip, paths claimed,
SLIMM_FORCE that puts the crafted block at a chunk start)}; INVALID(header, body) -> {name: (blob, the decoder's words)}.
Test infrastructure only."""
import struct
import zlib

import numpy as np

from tests.sam_deflate import gzip_frame


def _hand_made_fixed_block(symbols) -> bytes:
    """A raw DEFLATE stream of ONE fixed-Huffman block made by hand: symbols = [("lit", byte) | ("match", length, distance)].
    (zlib never emits a distance beyond the output; the writer wave has to refuse one.)"""
    bits = []
    def put(v, n):           # n bits, least significant first (extra bits, header)
        for k in range(n):
            bits.append((v >> k) & 1)
    def code(v, n):          # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            bits.append((v >> k) & 1)
    def litlen(s):
        if s < 144:
            code(0x30 + s, 8)
        elif s < 256:
            code(0x190 + (s - 144), 9)
        elif s < 280:
            code(s - 256, 7)
        else:
            code(0xc0 + (s - 280), 8)
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    dext = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
    put(1, 1)
    put(1, 2)                # BFINAL, fixed codes
    for s in symbols:
        if s[0] == "lit":
            litlen(s[1])
        else:
            _, length, dist = s
            li = max(i for i in range(29) if lbase[i] <= length)
            litlen(257 + li)
            put(length - lbase[li], lext[li])
            di = max(i for i in range(30) if dbase[i] <= dist)
            code(di, 5)
            put(dist - dbase[di], dext[di])
    litlen(256)
    while len(bits) % 8:
        bits.append(0)
    return bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    """A DEFLATE bit stream written by hand: put() = header fields / extra bits (least significant bit first), code() = a
    Huffman code (most significant bit first)."""
    def __init__(self):
        self.b = []

    def put(self, v, n):
        self.b += [(v >> k) & 1 for k in range(n)]

    def code(self, v, n):
        self.b += [(v >> k) & 1 for k in range(n - 1, -1, -1)]

    def align(self):
        while len(self.b) % 8:
            self.b.append(0)

    def bytes(self):
        self.align()
        return bytes(sum(self.b[i + k] << k for k in range(8)) for i in range(0, len(self.b), 8))


def _canonical(lengths):
    """RFC 1951 3.2.2: the canonical code of a list of code lengths (0 = unused) -> {symbol: (code, length)}."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def dynamic_block(bits: Bits, ll_len, d_len, tokens, final=True, cl_seq=None, hlit=None, hdist=None, end=True):
    """One dynamic-Huffman block with the GIVEN code lengths (ll_len: up to 288 literal/length, d_len: up to 32 distance) and
    tokens [int literal | (length, distance) | ("lsym", symbol, extra) | ("dsym", symbol, extra)].  cl_seq: the code-length
    symbols [(symbol, extra)] to send instead of one symbol per length (repeats: 16 / 17 / 18)."""
    hlit = len(ll_len) if hlit is None else hlit
    hdist = len(d_len) if hdist is None else hdist
    if cl_seq is None:
        cl_seq = [(l, 0) for l in list(ll_len[:hlit]) + list(d_len[:hdist])]
    used = sorted({s for s, _ in cl_seq})
    # a complete code over the code-length symbols in use: all of one length
    k = 1
    while (1 << k) < max(2, len(used)):
        k += 1
    cl_len = [0] * 19
    for s in used:
        cl_len[s] = k
    for s in range(19):          # fill the code up so that it is complete (unused symbols are harmless)
        if sum(1 for x in cl_len if x) == (1 << k):
            break
        if not cl_len[s]:
            cl_len[s] = k
    cl_code = _canonical(cl_len)
    hclen = max(i for i, s in enumerate(_CLORDER) if cl_len[s]) + 1
    bits.put(1 if final else 0, 1)
    bits.put(2, 2)
    bits.put(hlit - 257, 5)
    bits.put(hdist - 1, 5)
    bits.put(max(hclen, 4) - 4, 4)
    for i in range(max(hclen, 4)):
        bits.put(cl_len[_CLORDER[i]], 3)
    for s, extra in cl_seq:
        bits.code(*cl_code[s])
        if s == 16:
            bits.put(extra, 2)
        elif s == 17:
            bits.put(extra, 3)
        elif s == 18:
            bits.put(extra, 7)
    ll, dd = _canonical(list(ll_len)), _canonical(list(d_len))
    for t in tokens:
        if isinstance(t, int):
            bits.code(*ll[t])
        elif t[0] == "lsym":
            bits.code(*ll[t[1]])
        elif t[0] == "dsym":
            bits.code(*dd[t[1]])
        else:
            length, dist = t
            li = 28 if length == 258 else max(i for i in range(28) if _LBASE[i] <= length)
            bits.code(*ll[257 + li])
            bits.put(length - _LBASE[li], _LEXT[li])
            di = max(i for i in range(30) if _DBASE[i] <= dist)
            bits.code(*dd[di])
            bits.put(dist - _DBASE[di], _DEXT[di])
    if end:
        bits.code(*ll[256])


def _replay(tokens, start=b""):
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def _ll_lengths_15():
    """A COMPLETE literal/length code of 286 symbols with every length from 2 to 15 in use: one symbol each at 2 .. 14 and two at
    15 fill half the code space (the end-of-block code and length symbols among them), 241 more at 9 and 30 at 10 the other half."""
    l = [9] * 286
    for s in range(226, 256):
        l[s] = 10
    deep = [256, 257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 267, 268, 285, 284]
    for s, length in zip(deep, list(range(2, 15)) + [15, 15]):
        l[s] = length
    assert sum(2.0 ** -x for x in l) == 1.0
    return l


def _d_lengths_15():
    """... and of the 30 distance symbols: 2 .. 14 once, 15 twice, one at 4 and fourteen at 5."""
    l = [5] * 30
    l[0] = 4
    for s, length in zip(range(15, 30), list(range(2, 15)) + [15, 15]):
        l[s] = length
    assert sum(2.0 ** -x for x in l) == 1.0
    return l


def _lit_lengths(n_len_symbols):
    """A complete code for the 256 literals, the end-of-block code and the first n_len_symbols length symbols (1 or 3): literals
    0 .. 253 at 8 bits, the rest at 9 (1 symbol: 254, 255, 256, 257) or 254 / 255 at 9 and four codes of 10 behind them."""
    if n_len_symbols == 1:
        return [8] * 254 + [9, 9, 9, 9]
    assert n_len_symbols == 3
    return [8] * 254 + [9, 9, 10, 10, 10, 10]


def _fixed_bits(tokens, final):
    """The bits of one fixed-Huffman block (without padding)."""
    raw = _hand_made_fixed_block([("lit", t) if isinstance(t, int) else ("match", t[0], t[1]) for t in tokens])
    bits = [(byte >> k) & 1 for byte in raw for k in range(8)]
    bits[0] = 1 if final else 0
    n = 3 + 7      # header + the end-of-block code
    for t in tokens:
        if isinstance(t, int):
            n += 8 if t < 144 else 9
        else:
            li = 28 if t[0] == 258 else max(i for i in range(28) if _LBASE[i] <= t[0])
            di = max(i for i in range(30) if _DBASE[i] <= t[1])
            n += (7 if 257 + li < 280 else 8) + _LEXT[li] + 5 + _DEXT[di]
    return bits[:n]


def _unusual_streams():
    """[(name, raw DEFLATE bytes, expected output or None = invalid)]"""
    rng = np.random.default_rng(17)
    cases = []
    text = bytes(rng.integers(0, 254, 3000, dtype=np.uint8))
    l15, d15 = _ll_lengths_15(), _d_lengths_15()
    # 1. no distance code at all: HDIST = 1, its one length 0; literals only
    b = Bits()
    dynamic_block(b, _lit_lengths(1), [0], list(text))
    cases.append(("no distance code", b.bytes(), text))
    # 2. a single 1-bit distance code (incomplete, and allowed): as distance symbol 0, and as symbol 29 with distances up to the start
    toks = list(text[:200]) + [(3, 1)] * 5 + [(5, 1)]
    b = Bits()
    dynamic_block(b, _lit_lengths(3), [1], toks)
    cases.append(("one 1-bit distance code (symbol 0)", b.bytes(), _replay(toks)))
    far = bytes(rng.integers(0, 254, 30000, dtype=np.uint8))
    toks = list(far) + [(3, 24577), (4, 30000), (5, 24577 + 5000)]
    b = Bits()
    dynamic_block(b, _lit_lengths(3), [0] * 29 + [1], toks)
    cases.append(("one 1-bit distance code (symbol 29)", b.bytes(), _replay(toks)))
    # 3. 15-bit codes on both alphabets, EVERY literal, length symbol and distance symbol in use, 258 as 284 + 31, distance 32 768
    base = bytes(rng.integers(0, 256, 33000, dtype=np.uint8))
    toks = list(base) + list(range(256))
    for li in range(29):
        toks.append((_LBASE[li] + ((1 << _LEXT[li]) - 1 if li < 28 else 0), 1 + li * 7))
    for di in range(30):
        toks.append((3 + di, _DBASE[di] + ((1 << _DEXT[di]) - 1)))
    want = bytearray(_replay(toks))
    for _ in range(258):
        want.append(want[-32768])
    b = Bits()
    dynamic_block(b, l15, d15, toks, end=False)
    llc, ddc = _canonical(l15), _canonical(d15)
    b.code(*llc[284]); b.put(31, 5); b.code(*ddc[29]); b.put((1 << 13) - 1, 13); b.code(*llc[256])   # 227 + 31 = 258 at 24577 + 8191
    cases.append(("15-bit codes, every symbol", b.bytes(), bytes(want)))
    # 4. code-length repeats that cross the literal/length - distance boundary: a run of zeros (18), a run of equal lengths (16)
    ll4 = _lit_lengths(1) + [0] * 20                 # HLIT = 278: twenty zero lengths, then ten zero distance lengths, then a 1
    d4 = [0] * 10 + [1]
    seq = [(l, 0) for l in ll4[:258]] + [(18, 30 - 11), (1, 0)]        # 20 + 10 zeros in ONE run across the boundary
    toks = list(text[:500]) + [(3, 33)] * 3
    b = Bits()
    dynamic_block(b, ll4, d4, toks, cl_seq=seq)
    cases.append(("zero run across the HLIT boundary", b.bytes(), _replay(toks)))
    ll5 = [9] * 256 + [4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5]             # 1/2 + 4/16 + 8/32 = 1; lengths 3 .. 10 usable
    d5 = [5] * 28 + [4, 4]                           # 28/32 + 2/16 = 1
    seq = [(l, 0) for l in ll5[:264]]                # ... then 4 + 28 lengths of 5: five runs of six ACROSS the boundary, two singles
    seq += [(16, 3)] * 5 + [(5, 0), (5, 0), (4, 0), (4, 0)]
    toks = list(text[:300]) + [(5, 17), (9, 200)]
    b = Bits()
    dynamic_block(b, ll5, d5, toks, cl_seq=seq)
    cases.append(("repeat of a non-zero length across the HLIT boundary", b.bytes(), _replay(toks)))
    # 5. chains of self-overlapping 258-byte matches
    toks = [65, 66, 67] + [(258, 1)] * 20 + [(258, 2)] * 20 + [(258, 3)] * 20 + [68] + [(258, 258)] * 10
    b = Bits()
    dynamic_block(b, l15, d15, toks)
    cases.append(("chains of overlapping 258-byte matches", b.bytes(), _replay(toks)))
    # 6. several DEFLATE blocks: dynamic + EMPTY dynamic + fixed + dynamic, matches reaching back across the blocks; dynamic + stored + dynamic
    t1, t2, t3 = list(text[:700]), [(40, 650), (258, 700)], list(text[700:900]) + [(100, 1100)]
    b = Bits()
    dynamic_block(b, l15, d15, t1, final=False)
    dynamic_block(b, l15, d15, [], final=False)
    b.b += _fixed_bits(t2, final=False)
    dynamic_block(b, l15, d15, t3, final=True)
    cases.append(("dynamic + empty dynamic + fixed + dynamic", b.bytes(), _replay(t1 + t2 + t3)))
    b = Bits()
    dynamic_block(b, l15, d15, t1, final=False)
    b.put(0, 1); b.put(0, 2); b.align()
    stored = bytes(range(200))
    b.b += [(byte >> k) & 1 for byte in struct.pack("<HH", len(stored), len(stored) ^ 0xffff) + stored for k in range(8)]
    dynamic_block(b, l15, d15, [(150, 180), (30, 850)], final=True)
    cases.append(("dynamic + stored + dynamic", b.bytes(), _replay([(150, 180), (30, 850)], _replay(t1) + stored)))
    # 7. exactly 65 536 bytes out
    toks = [7] + [(258, 1)] * 254 + [(3, 1)]
    assert len(_replay(toks)) == 65536
    b = Bits()
    dynamic_block(b, l15, d15, toks)
    cases.append(("65 536 bytes out", b.bytes(), _replay(toks)))
    # ---- invalid streams
    b = Bits(); dynamic_block(b, [8] * 257, [1], [1, 2, 3])
    cases.append(("over-subscribed literal code", b.bytes(), None))
    b = Bits(); dynamic_block(b, [9] * 257, [1], [1, 2, 3])
    cases.append(("incomplete literal code", b.bytes(), None))
    b = Bits(); dynamic_block(b, _lit_lengths(1) + [0] * 30, [1], [1, 2, 3])
    b.b[3:8] = [1, 1, 1, 1, 1]                      # HLIT field 31 -> 288 codes: more than the 286 there are
    cases.append(("HLIT 288", b.bytes(), None))
    ll = _lit_lengths(1)
    b = Bits(); dynamic_block(b, ll, [1], [1, 2, 3], cl_seq=[(16, 0)] + [(l, 0) for l in ll[3:]] + [(1, 0)])
    cases.append(("repeat with no previous length", b.bytes(), None))
    b = Bits(); dynamic_block(b, ll5, [5] * 32, list(text[:50]))
    cases.append(("HDIST 32", b.bytes(), None))
    ll7 = [9] * 256 + [4, 4, 4, 4, 5, 5, 5, 5] + [6] * 7 + [0] * 15 + [6]      # 287 lengths: symbol 286 would get a code
    assert sum(2.0 ** -x for x in ll7 if x) == 1.0
    b = Bits(); dynamic_block(b, ll7, d5, list(text[:50]))
    cases.append(("HLIT 287", b.bytes(), None))
    # (the FIXED code has codes for distance symbols 30 / 31 and length symbols 286 / 287: using one is an error)
    b = Bits(); b.put(1, 1); b.put(1, 2)
    for ch in b"abcdefgh":
        b.code(0x30 + ch, 8)
    b.code(257 - 256, 7); b.code(30, 5); b.code(0, 7)
    cases.append(("distance symbol 30 (fixed code)", b.bytes(), None))
    b = Bits(); b.put(1, 1); b.put(1, 2)
    for ch in b"abcdefgh":
        b.code(0x30 + ch, 8)
    b.code(0xc0 + (286 - 280), 8); b.code(0, 5); b.code(0, 7)
    cases.append(("length symbol 286 (fixed code)", b.bytes(), None))
    b = Bits(); dynamic_block(b, l15, d15, list(text[:10]) + [(5, 11)])
    cases.append(("a distance one byte beyond the start", b.bytes(), None))
    b = Bits(); dynamic_block(b, l15, d15, list(text[:100]), final=False)
    cases.append(("no final block", b.bytes(), None))
    return cases


# ---- gzip framing, a writer over a SAM text, and the directed inputs -----------------------------------------------------
NAMES = ("first_copy_at_a_chunk_start", "copies_inside_a_chunk", "symbols_and_extra_bits", "code_length_code",
         "one_code_sets_and_empty_blocks", "stored_blocks", "dynamic_stored_dynamic")
INVALID_NAMES = ("block_type_3", "stored_lengths", "code_lengths_set_incomplete", "no_end_of_block", "distances_set_incomplete",
                 "no_code_of_a_one_code_literal_set", "no_code_of_a_one_code_distance_set", "data_check", "length_check",
                 "over-subscribed literal code", "incomplete literal code", "HLIT 288", "repeat with no previous length", "HDIST 32",
                 "HLIT 287", "distance symbol 30 (fixed code)", "length symbol 286 (fixed code)", "a distance one byte beyond the start")
EVERY_CANDIDATE = "gzip_chunk=1"    # (a chunk start at every non-final dynamic block whose literal/length code is complete)


def flat_lengths(symbols, size):
    """A complete code over the symbols (two at least) in an alphabet of `size`: lengths that differ by one at most."""
    m, k = len(symbols), 1
    assert m >= 2
    while (1 << k) < m:
        k += 1
    out = [0] * size
    for i, s in enumerate(sorted(symbols)):
        out[s] = k - 1 if i < (1 << k) - m else k
    return out


def _length_symbol(length):
    i = 28 if length == 258 else max(k for k in range(28) if _LBASE[k] <= length)
    return 257 + i, length - _LBASE[i]


def _distance_symbol(dist):
    i = max(k for k in range(30) if _DBASE[k] <= dist)
    return i, dist - _DBASE[i]


def _symbols(t):
    """A token int | (length, distance) | ("sym", length symbol, extra, distance symbol, extra) in symbols and as a copy."""
    if t[0] == "sym":
        return t[1:], (_LBASE[t[1] - 257] + t[2], _DBASE[t[3]] + t[4])
    return _length_symbol(t[0]) + _distance_symbol(t[1]), t


class Deflate:
    """A raw deflate stream written block by block over a text that is known beforehand: every block's tokens are replayed
    and, where `expect` is given, held against the text they are to give."""

    def __init__(self):
        self.b, self.text = Bits(), bytearray()

    def at(self):
        return len(self.b.b)

    def _replayed(self, tokens, expect):
        before = len(self.text)
        for t in tokens:
            if isinstance(t, int):
                self.text.append(t)
            else:
                length, dist = _symbols(t)[1]
                assert dist <= len(self.text), (length, dist, len(self.text))
                for _ in range(length):
                    self.text.append(self.text[-dist])
        assert expect is None or bytes(self.text[before:]) == expect, (bytes(self.text[before:])[:80], expect[:80])

    def dynamic(self, tokens, final=False, expect=None, ll_len=None, d_len=None, cl_seq=None):
        copies = [_symbols(t)[0] for t in tokens if not isinstance(t, int)]
        if ll_len is None:
            need = {t for t in tokens if isinstance(t, int)} | {c[0] for c in copies} | {256}
            ll_len = flat_lengths(need | ({0} if len(need) < 2 else set()), 286)
            ll_len = ll_len[:max(257, max(s for s in range(286) if ll_len[s]) + 1)]
        if d_len is None:
            need = {c[2] for c in copies}
            d_len = flat_lengths(need | ({0, 1} - need if len(need) < 2 else set()), 30) if need else [0]
            d_len = d_len[:max(s for s in range(len(d_len)) if d_len[s] or s == 0) + 1]
        dynamic_block(self.b, ll_len, d_len, [], final=final, cl_seq=cl_seq, end=False)
        ll, dd = _canonical(list(ll_len)), _canonical(list(d_len))
        for t in tokens:
            if isinstance(t, int):
                self.b.code(*ll[t])
            else:
                ls, le, ds, de = _symbols(t)[0]
                self.b.code(*ll[ls])
                self.b.put(le, _LEXT[ls - 257])
                self.b.code(*dd[ds])
                self.b.put(de, _DEXT[ds])
        self.b.code(*ll[256])
        self._replayed(tokens, expect)
        return self

    def fixed(self, tokens, final=False, expect=None):
        self.b.b += _fixed_bits(tokens, final)
        self._replayed(tokens, expect)
        return self

    def stored(self, data: bytes, final=False):
        self.b.put(1 if final else 0, 1)
        self.b.put(0, 2)
        self.b.align()
        self.b.b += [(byte >> k) & 1 for byte in struct.pack("<HH", len(data), len(data) ^ 0xffff) + data for k in range(8)]
        self.text += data
        return self

    def member(self):
        return gzip_frame(self.b.bytes(), bytes(self.text))


def bgzf_block(text: bytes, raw: bytes) -> bytes:
    """One BGZF block around a raw deflate stream of `text` (at most 65 536 bytes)."""
    bsize = 12 + 6 + len(raw) + 8
    assert len(text) <= 65536 and bsize <= 65536, (len(text), bsize)
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, (bsize - 1) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text))


# (a BGZF block holds at most 65 536 bytes of text: the input whose subject is a stored block of 65 535 bytes, behind a header, does not fit)
NOT_IN_BGZF = ("stored_blocks",)


def as_bgzf(inputs):
    """{name: (BGZF blocks, text, skip)}: every input's deflate stream as one BGZF block, the end-of-file block behind it."""
    return {name: (bgzf_block(text, blob[10:-8]) + bgzf_block(b"", b"\x03\x00"), text, skip)
            for name, (blob, text, skip, _, _) in inputs.items() if name not in NOT_IN_BGZF}


def _letters(n, seed, alphabet=b"ACGTNacgtn0123456789"):
    rng = np.random.default_rng(seed)
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _a_runs(text: bytes, least=100):
    """(start, end) of the text's runs of at least `least` 'A' (the SEQ fields of its records)."""
    out, p = [], text.find(b"A" * least)
    while p >= 0:
        q = p
        while q < len(text) and text[q] == 65:
            q += 1
        out.append((p, q))
        p = text.find(b"A" * least, q)
    return out


def INPUTS(header: bytes, body: bytes):
    out = {}
    whole = header + body
    runs = _a_runs(whole)

    def add(name, z, skip, paths, force):
        text = bytes(z.text)
        assert text[skip:] == body and text[:skip].startswith(header) and text[:skip].endswith(b"\n"), name
        blob = z.member()
        assert zlib.decompress(blob, 31) == text, name
        out[name] = (blob, text, skip, paths, force)

    # -- the first copy of a chunk, at n = 0, at distance 1, 2, 3, 7, 8 and 9; distance 5 across the chunk's start; a copy that
    #    lies wholly in front; the rest of each run a copy at distance 1 of bytes that are themselves unresolved
    #    -- over filler of period d, whose d bytes differ, and over the records' runs of one byte
    z, p = Deflate(), len(header)
    z.dynamic(list(header))
    for d in (2, 3, 5, 7, 8, 9):
        line = b"@CO\t" + (b"abcdefghi"[:d] * 30)[:d + 2 + 30 + 5] + b"\n"
        cut, n = 4 + d + 2, 20 if d == 5 else 30
        z.dynamic(list(line[:cut]))
        z.dynamic([(n, d)] + list(line[cut + n:]), expect=line[cut:])
    first_skip = len(z.text)
    for (s, e), first in zip(runs, [[(30, d)] for d in (1, 2, 3, 7, 8, 9)] + [[(20, 5)], [(5, 9), (10, 3)]]):
        z.dynamic(list(whole[p:s + 12]), expect=whole[p:s + 12])
        p = s + 12
        rest = e - p - sum(t[0] for t in first)
        z.dynamic(first + [(rest, 1)], expect=whole[p:e])   # (ends with the run: the next block starts the next chunk)
        p = e
    z.dynamic(list(whole[p:]), expect=whole[p:]).fixed([], final=True)
    add("first_copy_at_a_chunk_start", z, first_skip,
        ["copy:across_start:dist<8", "copy:across_start:dist>=8", "copy:wholly_in_front", "copy:of_unresolved", "copy:inside:dist1", "copy:inside:dist3",
         "bytes:from_in_front_of_chunk", "fixed:final", "fixed:empty", "dynamic:not_final", "set:lit:complete"], EVERY_CANDIDATE)
    # -- copies inside a chunk at distance 1 .. 7, 8 and 9 and more, with every tail of 1 .. 7 behind the eights
    #    -- each over a pattern of its distance's period, whose bytes differ
    z = Deflate()
    z.dynamic(list(header))
    tokens = list(b"@CO\t")
    for n, d in [(10 + d, d) for d in range(1, 8)] + [(9, 8), (10, 8), (11, 9), (12, 9), (13, 8), (14, 10), (15, 8)]:
        tokens += list(b"abcdefghij"[:d]) + [(n, d), ord("|")]
    z.dynamic(tokens + list(b"\n" + body))
    z.dynamic([], final=True, ll_len=[0] * 256 + [1], d_len=[0])
    add("copies_inside_a_chunk", z, len(z.text) - len(body),
        [f"copy:inside:dist{d}" for d in range(1, 9)] + ["copy:inside:dist>8"] + [f"copy:tail:{k}" for k in range(1, 8)]
        + ["dynamic:final", "dynamic:empty", "set:lit:one_code", "set:dist:none"], EVERY_CANDIDATE)
    # -- every length and distance symbol with its extra bits all zeros and all ones, codes of 2 .. 15 bits on both alphabets, 258
    #    as symbol 285 and as 284 + 31; the chunk's first copy at distance 32 768 from n = 0
    z = Deflate()
    l15, d15 = _ll_lengths_15(), _d_lengths_15()
    front = header + b"@CO\t" + _letters(33_000, 21)
    z.dynamic(list(front), ll_len=l15, d_len=[0])
    tokens = [(258, 32_768)]
    for k in range(30):
        li = k % 29
        tokens += [("sym", 257 + li, 0, k, 0), ("sym", 257 + li, (1 << _LEXT[li]) - 1, k, (1 << _DEXT[k]) - 1)]
    tokens += [("sym", 284, 31, 29, 8191)]
    z.dynamic(tokens + list(b"\n" + body), ll_len=l15, d_len=d15)
    z.fixed([], final=True)
    skip = len(z.text) - len(body)
    add("symbols_and_extra_bits", z, skip,
        [f"len_sym:{s}:{e}" for s in range(257, 286) for e in ("zeros", "ones")] + [f"dist_sym:{s}:{e}" for s in range(30) for e in ("zeros", "ones")]
        + ["len258:as_285", "len258:as_284+31", "copy:dist32768_from_n0", "hlit:286", "hdist:30", "hclen:19", "copy:wholly_in_front"]
        + [f"lit_len:{k}" for k in range(2, 16)] + [f"dist_len:{k}" for k in range(2, 16)], EVERY_CANDIDATE)
    # -- the code-length code: lengths 1 .. 15 on both alphabets; 16, 17 and 18 at their least and greatest repeat; HLIT 257, HDIST 1;
    #    a repeat across the HLIT boundary
    z = Deflate()
    z.dynamic(list(header + b"@CO\t"))
    few = b"ACGTNacgtn0123"
    ll = [0] * 258
    for s, ln in zip(sorted(few) + [256, 257], list(range(1, 16)) + [15]):
        ll[s] = ln
    z.dynamic(list(_letters(40, 22, few)) + [(3, 5), (3, 6)], ll_len=ll, d_len=list(range(1, 16)) + [15])
    # (literals 3, 14, 26 .. 38 and 177: zero runs of exactly 3, 10, 11 and 138 in front of them, equal lengths seven and four times)
    ll = [0] * 257
    for s in [3, 14, 26] + list(range(27, 34)) + list(range(35, 39)) + [256]:
        ll[s] = 4
    ll[34] = ll[177] = 5
    seq = [(17, 0), (4, 0), (17, 7), (4, 0), (18, 0), (4, 0), (4, 0), (16, 3), (5, 0), (4, 0), (16, 0), (18, 127), (5, 0), (18, 78 - 11), (4, 0), (0, 0)]
    odd = bytes([3, 14, 26] + list(range(27, 39)) + [177]) * 2
    z.dynamic(list(odd), ll_len=ll, d_len=[0], cl_seq=seq)
    used = sorted(set(b"\n@CO\t" + few))
    ll = flat_lengths(used + [256, 257], 258) + [0] * 20
    seq = [(ln, 0) for ln in ll[:258]] + [(18, 30 - 11), (1, 0)]     # (twenty zeros, and ten more on the other side, in ONE run)
    z.dynamic(list(b"\n@CO\t" + _letters(60, 23, few)) + [(3, 33)] * 3, ll_len=ll, d_len=[0] * 10 + [1], cl_seq=seq)
    z.dynamic(list(b"\n" + body), final=True)
    skip = len(z.text) - len(body)
    add("code_length_code", z, skip,
        [f"cl:{k}" for k in range(16)] + ["cl:16:rep3", "cl:16:rep6", "cl:17:rep3", "cl:17:rep10", "cl:18:rep11", "cl:18:rep138", "cl:repeat_across_hlit",
                                         "hlit:257", "hdist:1", "lit_len:1", "dist_len:1", "set:dist:none", "set:dist:one_code", "lit:from_144", "dynamic:final"], None)
    # -- the one-code literal set (the end of the block only), the one-code distance set, no distance code; empty blocks of both
    #    kinds, an empty dynamic block in front of a fixed one
    z = Deflate()
    half = len(header) + len(body) // 2
    z.dynamic(list(header), d_len=[0])
    z.dynamic([], ll_len=[0] * 256 + [1], d_len=[0])
    z.fixed(list(whole[len(header):half]))
    z.fixed([])
    (s, e) = [r for r in runs if r[0] > half][0]
    z.dynamic(list(whole[half:s + 10]) + [(e - s - 10, 1)], d_len=[1])
    z.dynamic(list(whole[e:]), expect=whole[e:])
    z.dynamic([], final=True, ll_len=[0] * 256 + [1], d_len=[0])
    add("one_code_sets_and_empty_blocks", z, len(header),
        ["set:lit:one_code", "set:dist:one_code", "set:dist:none", "dynamic:empty", "fixed:empty", "fixed:not_final", "dynamic:final", "lit:below_144"], None)
    # -- stored blocks of 0 and 65 535 bytes, and behind 0 .. 7 pad bits (a fixed block of j literals of 9 bits in front of each)
    z = Deflate()
    z.fixed(list(header + b"@CO\t"))
    z.stored(_letters(65_535, 24)).stored(b"")
    z.fixed(list(b"\n@CO\t"))
    for j in range(8):
        z.fixed([0xc0] * j).stored(b"|%d|" % j)
    z.fixed(list(b"\n" + body), final=True)
    skip = len(z.text) - len(body)
    add("stored_blocks", z, skip, ["stored:len:0", "stored:len:65535"] + [f"stored:pad:{k}" for k in range(8)] + ["lit:from_144", "fixed:final", "fixed:not_final"], None)
    # -- dynamic + stored + dynamic in ONE chunk: copies into the stored bytes, into the dynamic block in front of them and in front of the chunk
    z = Deflate()
    r = runs
    lines = [whole.index(b"\n", r[k][1]) + 1 for k in range(len(r))]     # (where the line behind run k starts)
    z.dynamic(list(whole[:lines[3]]), expect=whole[:lines[3]])
    z.dynamic(list(whole[lines[3]:r[4][0]]) + [(100, r[4][0] - r[3][0])] + list(whole[r[4][1]:lines[5]]), expect=whole[lines[3]:lines[5]])
    z.stored(whole[lines[5]:lines[8]])
    tokens = list(whole[lines[8]:r[9][0]]) + [(100, r[9][0] - r[8][0])] + list(whole[r[9][1]:r[10][0]]) + [(100, r[10][0] - r[4][0])]
    tokens += list(whole[r[10][1]:r[11][0]]) + [(100, r[11][0] - r[2][0])] + list(whole[r[11][1]:])
    z.dynamic(tokens, final=True, expect=whole[lines[8]:])
    add("dynamic_stored_dynamic", z, len(header),
        ["copy:from_stored_block", "copy:from_earlier_block_of_chunk", "copy:wholly_in_front", "dynamic:final", "bytes:from_in_front_of_chunk"], EVERY_CANDIDATE)
    assert tuple(out) == NAMES, list(out)
    return out


def INVALID(header: bytes, body: bytes):
    """{name: (gzip bytes, the words of gz::status_text)}: one variant per status from kBadBlockType to kBadLength -- but
    kOverrun, a guard of the buffers that no stream reaches: the size pass and the decode pass read the same bits -- the
    invalid streams of _unusual_streams among them (those stand alone: one of them is invalid only at a member's start)."""
    out = {}
    whole = header + body

    def behind_the_text(write):
        z = Deflate()
        z.dynamic(list(whole))
        write(z)
        return gzip_frame(z.b.bytes(), whole)

    def type_3(z):
        z.b.put(1, 1)
        z.b.put(3, 2)
    out["block_type_3"] = (behind_the_text(type_3), "invalid block type")

    def stored(z):
        z.b.put(1, 1)
        z.b.put(0, 2)
        z.b.align()
        z.b.b += [(byte >> k) & 1 for byte in struct.pack("<HH", 3, 3 ^ 0xfffe) + b"abc" for k in range(8)]
    out["stored_lengths"] = (behind_the_text(stored), "invalid stored block lengths")

    def header_bits(z, hlit, hdist, cl):
        z.b.put(1, 1)
        z.b.put(2, 2)
        z.b.put(hlit - 257, 5)
        z.b.put(hdist - 1, 5)
        z.b.put(19 - 4, 4)
        for s in _CLORDER:
            z.b.put(cl[s], 3)

    def cl_incomplete(z):   # (two codes of two bits: half the code space is left)
        header_bits(z, 257, 1, [2 if s in (0, 8) else 0 for s in range(19)])
        z.b.put(0, 64)
    out["code_lengths_set_incomplete"] = (behind_the_text(cl_incomplete), "invalid code lengths set")

    def lengths(z, ll_len, d_len, bits=()):
        dynamic_block(z.b, ll_len, d_len, [], end=False)
        z.b.b += list(bits) + [0] * 64
    out["no_end_of_block"] = (behind_the_text(lambda z: lengths(z, [8] * 256 + [0], [0])), "invalid code -- missing end-of-block")
    out["distances_set_incomplete"] = (behind_the_text(lambda z: lengths(z, _lit_lengths(1), [2, 2])), "invalid distances set")
    out["no_code_of_a_one_code_literal_set"] = (behind_the_text(lambda z: lengths(z, [0] * 256 + [1], [0], [1])), "invalid literal/length code")
    ll = _lit_lengths(1)
    code = _canonical(ll)
    def one_distance(z):
        dynamic_block(z.b, ll, [1], [65, 66, 67], end=False)
        z.b.code(*code[257])
        z.b.put(1, 1)      # (the one distance code is the bit 0)
        z.b.put(0, 64)
    out["no_code_of_a_one_code_distance_set"] = (behind_the_text(one_distance), "invalid distance code")
    z = Deflate()
    z.dynamic(list(whole), final=True)
    out["data_check"] = (gzip_frame(z.b.bytes(), whole, crc=zlib.crc32(whole) ^ 1), "incorrect data check")
    out["length_check"] = (gzip_frame(z.b.bytes(), whole, isize=len(whole) + 1), "incorrect length check")
    words = {"over-subscribed literal code": "invalid literal/lengths set", "incomplete literal code": "invalid literal/lengths set",
             "HLIT 288": "too many length or distance symbols", "repeat with no previous length": "invalid bit length repeat",
             "HDIST 32": "too many length or distance symbols", "HLIT 287": "too many length or distance symbols",
             "distance symbol 30 (fixed code)": "invalid distance code", "length symbol 286 (fixed code)": "invalid literal/length code",
             "a distance one byte beyond the start": "invalid distance too far back"}
    for name, raw, want in _unusual_streams():
        if want is None and name in words:
            out[name] = (gzip_frame(raw, b""), words[name])
    assert tuple(out) == INVALID_NAMES, list(out)
    return out
