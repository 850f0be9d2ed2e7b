"""bzip2 streams written on purpose, one path family of the block decoder (slimm_amd/csrc/bzip2_block.h, bzip2_decode.hip) each:
a writer of the format's every layer -- RLE1 with a chosen run cap, a BWT with a choice among equal rotations for origPtr, MTF
and RUNA / RUNB, chosen code lengths per table (under-subscribed sets are legal), a chosen table count, selector pattern and
surplus selectors, canonical codes, an MSB-first bit writer, block and combined CRC -- and the inputs made with it.  Every
input is the SAM text it is given, with filler that is no SAM in @CO header lines; tests/bzip2_paths.py shows which paths
each reaches.  INPUTS(header, body) -> {name: (blob, text, skip, paths claimed, SLIMM_FORCE for a round per push)};
INVALID(header, body) -> {name: (blob, the decoder's words)}: one rule broken each.  Test infrastructure only."""
import heapq
import random

import numpy as np

from tests.bzip2_paths import BLOCK_MAGIC, EOS_MAGIC, crc32_bzip2

FORCE = "bzip2_round=1"
NAMES = ("tables_and_selectors", "surplus_selectors", "code_lengths", "rle1_counts", "block_edges_in_runs", "block_sizes",
         "every_byte_value", "orig_ptrs", "periods", "levels_and_streams", "long_runs", "eob_and_run_positions")
INVALID_NAMES = ("randomised", "no_byte_in_use", "tables_0", "tables_1", "tables_7", "selectors_0", "selector_past_the_tables",
                 "start_length_0", "start_length_21", "step_below_1", "step_above_20", "no_code_of_an_incomplete_set",
                 "symbols_beyond_the_selectors", "run_digit_2_20", "n_above_the_level", "run_overshoots", "orig_ptr_n", "block_crc",
                 "combined_crc", "count_byte_missing")


class BitWriter:
    """Bits, the most significant first."""

    def __init__(self):
        self.parts = []

    def put(self, v, k):
        if k:
            self.parts.append(format(v, "0%db" % k))

    def raw(self, bits: str):
        self.parts.append(bits)

    def to_byte(self):
        n = sum(len(p) for p in self.parts)
        self.parts.append("0" * (-n % 8))

    def bytes(self):
        s = "".join(self.parts)
        assert len(s) % 8 == 0
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def rle1(text: bytes, cap: int = 255) -> bytes:
    """Runs of 4 .. cap equal bytes as four of them and a count byte (cap 255: what bzip2 writes; 259: count bytes up to 255)."""
    out, i, n = bytearray(), 0, len(text)
    while i < n:
        j = i
        while j < n and text[j] == text[i] and j - i < cap:
            j += 1
        out += text[i:i + 1] * min(4, j - i)
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def un_rle1(s: bytes) -> bytes:
    out, i = bytearray(), 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] == s[i] and j - i < 4:
            j += 1
        out += s[i:j]
        if j - i == 4 and j < len(s):
            out += s[i:i + 1] * s[j]
            j += 1
        i = j
    return bytes(out)


def bwt(s: bytes, pick: int = 0):
    """(the last column of the sorted rotations of s, origPtr): rotation 0's place among them -- where several rotations
    equal it (a text that repeats itself), the pick-th of their places."""
    n = len(s)
    a = np.frombuffer(s, dtype=np.uint8).astype(np.int64)
    rank, idx, k = a.copy(), np.arange(n), 1
    while True:   # prefix doubling over the rotations
        key = rank * (int(rank.max()) + 1) + rank[(idx + k) % n]
        order = np.argsort(key, kind="stable")
        sk = key[order]
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.concatenate(([0], np.cumsum(sk[1:] != sk[:-1])))
        k *= 2
        if k >= n or int(rank.max()) == n - 1:
            break
    order = np.argsort(rank, kind="stable")
    same = np.flatnonzero(rank[order] == rank[0])
    return a[(order - 1) % n].astype(np.uint8).tobytes(), int(same[pick])


def run_digits(run: int):
    """A run's length in RUNA (0) / RUNB (1) digits: bijective base 2, the lowest first."""
    out = []
    while run:
        out.append(0 if run & 1 else 1)
        run = (run - (1 if run & 1 else 2)) >> 1
    return out


def mtf_runs(ll: bytes):
    """(the byte values in use, the symbols: 0 RUNA, 1 RUNB, k + 1 an MTF index k, the end of the block last)."""
    used = sorted(set(ll))
    at = {b: i for i, b in enumerate(used)}
    order, syms, run = list(range(len(used))), [], 0

    def flush(run):
        syms.extend(run_digits(run))

    for b in ll:
        u = at[b]
        if order[0] == u:
            run += 1
            continue
        flush(run)
        run = 0
        j = order.index(u)
        syms.append(j + 1)
        order.insert(0, order.pop(j))
    flush(run)
    return used, syms + [len(used) + 1]


def huffman_lengths(freq, limit=17):
    """Code lengths of a Huffman code over every symbol (a frequency of 0 counts as 1), none above `limit`."""
    freq = [max(1, f) for f in freq]
    while True:
        heap = [(f, i, (i,)) for i, f in enumerate(freq)]
        heapq.heapify(heap)
        lens, tick = [0] * len(freq), len(freq)
        if len(heap) == 1:
            return [1]
        while len(heap) > 1:
            fa, _, sa = heapq.heappop(heap)
            fb, _, sb = heapq.heappop(heap)
            for s in sa + sb:
                lens[s] += 1
            heapq.heappush(heap, (fa + fb, tick, sa + sb))
            tick += 1
        if max(lens) <= limit:
            return lens
        freq = [(f >> 1) | 1 for f in freq]


class Block:
    """One block of `text` (or of the RLE1 string rle, whatever RLE1 encoder wrote it); its fields may be changed before
    emit(): tables (code lengths per symbol, one list per table), selectors (a table per 50 symbols), n_sel (the count
    written: surplus selectors name table 0), starts (a table's 5-bit start length), detours ({(table, symbol): steps
    +1 / -1 taken before the length is settled}), and, for invalid variants, the header fields themselves."""

    def __init__(self, text: bytes = None, cap: int = 255, pick: int = 0, rle: bytes = None, n_tables: int = 2):
        self.rle = rle1(text, cap) if rle is None else rle
        self.text = un_rle1(self.rle) if text is None else text
        self.ll, self.orig = bwt(self.rle, pick)
        self.used, self.syms = mtf_runs(self.ll)
        self.crc = crc32_bzip2(self.text)
        self.n = len(self.rle)
        self.randomised = 0
        self.alpha = len(self.used) + 2
        freq = [0] * self.alpha
        for s in self.syms:
            freq[s] += 1
        self.tables = [huffman_lengths(freq) for _ in range(n_tables)]
        self.groups = (len(self.syms) + 49) // 50
        self.selectors = [g % n_tables for g in range(self.groups)]
        self.n_sel = self.n_tables_field = None
        self.starts, self.detours, self.unary, self.raw_symbol = {}, {}, {}, {}

    def emit(self, w: BitWriter):
        w.put(BLOCK_MAGIC, 48)
        w.put(self.crc, 32)
        w.put(self.randomised, 1)
        w.put(self.orig, 24)
        rows = [sum(1 << (15 - j) for j in range(16) if 16 * i + j in self.used) for i in range(16)]
        w.put(sum(1 << (15 - i) for i in range(16) if rows[i]), 16)
        for row in rows:
            if row:
                w.put(row, 16)
        nt = len(self.tables)
        w.put(nt if self.n_tables_field is None else self.n_tables_field, 3)
        n_sel = len(self.selectors) if self.n_sel is None else self.n_sel
        w.put(n_sel, 15)
        order = list(range(nt))
        for i in range(n_sel):
            s = self.selectors[i] if i < len(self.selectors) else 0
            j = order.index(s)
            order.insert(0, order.pop(j))
            w.raw("1" * self.unary.get(i, j) + ("0" if i not in self.unary else ""))
        codes = []
        for t, lens in enumerate(self.tables):
            cur = self.starts.get(t, lens[0])
            w.put(cur, 5)
            for i, ln in enumerate(lens):
                for step in self.detours.get((t, i), []):
                    w.put(2 if step > 0 else 3, 2)
                    cur += step
                while cur != ln:
                    w.put(2 if cur < ln else 3, 2)
                    cur += 1 if cur < ln else -1
                w.put(0, 1)
            code, table = 0, {}
            for ln in range(min(lens), max(lens) + 1):   # the canonical code: by length, then by symbol
                for s in range(len(lens)):
                    if lens[s] == ln:
                        table[s] = format(code, "0%db" % ln)
                        code += 1
                code <<= 1
            codes.append(table)
        for k, s in enumerate(self.syms):
            g = k // 50
            w.raw(self.raw_symbol.get(k) or codes[self.selectors[g] if g < len(self.selectors) else 0][s])


def stream(blocks, level=9) -> bytes:
    """One stream of the blocks (Block objects), bit-packed, with its end-of-stream marker and combined CRC."""
    w, combined = BitWriter(), 0
    w.put(0x425a68, 24)
    w.put(48 + level, 8)
    for b in blocks:
        b.emit(w)
        combined = (((combined << 1) | (combined >> 31)) & 0xffffffff) ^ b.crc
    w.put(EOS_MAGIC, 48)
    w.put(combined, 32)
    w.to_byte()
    return w.bytes()


def pieces(text: bytes, cuts):
    bounds = [0] + sorted(c for c in set(cuts) if 0 < c < len(text)) + [len(text)]
    return [text[a:b] for a, b in zip(bounds, bounds[1:])]


def letters(n: int, seed: int, alphabet: bytes = b"ACGTNacgtn012345678") -> bytes:
    """n bytes of the alphabet, no two neighbours equal (RLE1 leaves them alone)."""
    rng, out = random.Random(seed), bytearray()
    while len(out) < n:
        c = rng.choice(alphabet)
        if not out or c != out[-1]:
            out.append(c)
    return bytes(out)


def _a_runs(body: bytes, least=100):
    """Where the body's runs of at least `least` 'A' start (the SEQ fields of its records)."""
    out, p = [], body.find(b"A" * least)
    while p >= 0:
        q = p
        while q < len(body) and body[q] == 65:
            q += 1
        out.append((p, q))
        p = body.find(b"A" * least, q)
    return out


def INPUTS(header: bytes, body: bytes):
    out = {}
    whole = header + body

    def add(name, blob, text, skip, paths):
        assert text[skip:] == body and text[:skip].startswith(header) and text[:skip].endswith(b"\n"), name
        out[name] = (blob, text, skip, paths, FORCE)

    def filled(payloads):
        """(the text with one @CO line per payload behind the header, where each payload starts in it)."""
        text, at = bytearray(header), []
        for p in payloads:
            text += b"@CO\t"
            at.append(len(text))
            text += p + b"\n"
        return bytes(text) + body, at, len(text)

    # -- 2 .. 6 tables; selectors at every MTF position; a table no selector names
    cut = pieces(whole, [len(whole) * k // 10 for k in (1, 2, 3, 4)])
    blocks = [Block(p, n_tables=nt) for p, nt in zip(cut, (2, 3, 4, 5, 6))]
    blocks[1].selectors = [g % 2 for g in range(blocks[1].groups)]
    assert blocks[4].groups >= 12
    add("tables_and_selectors", stream(blocks), whole, len(header),
        [f"tables:{k}" for k in range(2, 7)] + [f"sel_mtf:{k}" for k in range(6)] + ["table:unselected", "n_sel:exact", "streams:1", "level:9", "bwt:cycles:1"])
    # -- more selectors than the block needs: a few, and more than 18 002 (read and dropped)
    blocks = [Block(p) for p in pieces(whole, [len(whole) // 2])]
    blocks[0].n_sel, blocks[1].n_sel = blocks[0].groups + 7, 18_010
    add("surplus_selectors", stream(blocks), whole, len(header), ["n_sel:surplus", "n_sel:above_18002"])
    # -- code lengths 1 .. 20 in one table (every extension of a code of min_len bits), 20 .. 1 in another, all equal in a third
    text, at, skip = filled([letters(900, 3)])
    cut = pieces(text, [at[0], at[0] + 900])
    b = Block(cut[1], n_tables=3)
    assert b.alpha == 21 and set(b.syms) == set(range(21)), "every symbol of the 21 is to occur"
    b.tables = [list(range(1, 21)) + [20], [20] + list(range(20, 0, -1)), [5] * 21]
    b.detours = {(0, 3): [+1, +1, -1, -1], (2, 7): [-1, +1]}
    add("code_lengths", stream([Block(cut[0]), b, Block(cut[2])]), text, skip,
        ["len_start:1", "len_start:20", "len_step:up", "len_step:down", "len_step:both_in_one_symbol", "len_used:1", "len_used:20", "len:min_eq_max", "tables:3"]
        + [f"ext:{k}" for k in range(20)])
    # -- RLE1's count bytes: 0, 1, 251 and, under a run cap of 259, 252 .. 255; a run that goes on behind its count byte
    runs = b"".join(bytes([c]) * n for c, n in zip(b"abcdefg", (4, 5, 255, 256, 257, 258, 259)))
    text, at, skip = filled([runs + b"h" * 600, b"i" * 600 + b"jjjjkkkkk"])
    cut = pieces(text, [at[1] - 5])
    add("rle1_counts", stream([Block(cut[0], cap=259), Block(cut[1])]), text, skip,
        [f"rle1:count:{k}" for k in (0, 1, 251, 252, 253, 254, 255)] + ["rle1:byte_behind_count_is_the_runs"])
    # -- blocks that end inside a run: 1, 2, 3 equal bytes with the same byte first in the next block; four and a count
    a = _a_runs(body)
    cuts = [len(header) + a[0][0] + 1, len(header) + a[1][0] + 2, len(header) + a[2][0] + 3, len(header) + a[3][0] + 50, len(header) + a[4][1]]
    add("block_edges_in_runs", stream([Block(p) for p in pieces(whole, cuts)]), whole, len(header),
        [f"rle1:block_ends_in:{k}:next_begins_same" for k in (1, 2, 3)] + ["rle1:block_ends_in_4_and_count"])
    # -- blocks of 1, 255, 256 and 257 bytes
    text, at, skip = filled([letters(1 + 255 + 256 + 257, 5)])
    cut = pieces(text, [at[0], at[0] + 1, at[0] + 256, at[0] + 512, at[0] + 769])
    add("block_sizes", stream([Block(p) for p in cut]), text, skip, ["n:1", "n:255", "n:256", "n:257", "used:1", "map:groups:1", "orig:0", "orig:n-1", "run:at_block_start"])
    # -- every byte value in use: 16 groups of the map, MTF index 255 (a line feed inside the filler starts a new @CO line)
    rng, every = random.Random(11), bytearray()
    for _ in range(12):
        perm = list(range(256))
        rng.shuffle(perm)
        for v in perm:
            every += b"\n@CO\t" if v == 10 else bytes([v])
    text, at, skip = filled([bytes(every)])
    cut = pieces(text, [at[0], at[0] + len(every)])
    add("every_byte_value", stream([Block(p) for p in cut]), text, skip, ["used:256", "map:groups:16", "mtf:255", "mtf:1"])
    # -- origPtr 0, n - 1, on a multiple of 256 and off one
    low = b"\x01" + letters(300, 7)
    high = b"~" + letters(300, 8)
    ruler = b"M" + letters(256, 9, b"ABCDEFGHIJKL") + letters(60, 10, b"NOPQRSTUVWXYZ")
    text, at, skip = filled([low, high, ruler])
    cut = pieces(text, [at[0], at[0] + len(low), at[1], at[1] + len(high), at[2], at[2] + len(ruler)])
    blocks = [Block(p) for p in cut]
    assert (blocks[1].orig, blocks[3].orig, blocks[5].orig) == (0, 300, 256)
    add("orig_ptrs", stream(blocks), text, skip, ["orig:0", "orig:n-1", "orig:ruler", "orig:off_ruler"])
    # -- texts that repeat themselves: period 1 (an RLE1 string of five equal bytes), period 2, a line two and three times;
    #    origPtr the first and the last of the equal rotations
    twice, thrice = letters(150, 12) + b"\n@CO\t", letters(70, 13) + b"\n@CO\t"
    text, at, skip = filled([b"ab" * 300, b"ba" * 300, twice * 2 + b"2", thrice * 3 + b"3"])
    h = skip
    cuts = [at[0], at[0] + 600, at[1], at[1] + 600, at[2], at[2] + 2 * len(twice), at[3], at[3] + 3 * len(thrice),
            h + a[0][0] + 3, h + a[0][0] + 3 + 69, h + a[1][0] + 1, h + a[1][0] + 1 + 69]
    cut = pieces(text, cuts)
    picks = {1: 0, 3: -1, 5: -1, 7: 0, 9: 0, 11: -1}
    blocks = [Block(p, pick=picks.get(i, 0)) for i, p in enumerate(cut)]
    assert blocks[9].rle == b"AAAAA" and blocks[11].orig == 4 and blocks[3].orig != blocks[1].orig
    add("periods", stream(blocks), text, skip, ["bwt:period:1", "bwt:period:2", "bwt:cycles:2", "bwt:cycles:3", "bwt:cycles:1"])
    # -- a stream per level, an empty stream among them
    cut = pieces(whole, [len(whole) * k // 9 for k in range(1, 9)])
    blob = b"".join(stream([Block(p)], level=k + 1) + (stream([], 3) if k == 4 else b"") for k, p in enumerate(cut))
    add("levels_and_streams", blob, whole, len(header), [f"level:{k}" for k in range(1, 10)] + ["streams:many", "stream:empty"])
    # -- RUNA and RUNB at every weight a block of level 1 can hold: zero runs of 98 303 (fifteen RUNA and RUNB at 2^15), 65 535
    #    (sixteen RUNA) and 65 534 (fifteen RUNB); a block of exactly 100 000 bytes whose last symbols are a run
    x = b"\x01"   # (the run's byte, and the count byte 1 behind every four of them: five bytes of RLE1 for five of text)
    tails = [letters(100_000 - 98_305, 14), letters(999, 15), letters(998, 16)]
    rles = [x * 98_305 + tails[0], x * 65_537 + tails[1], x * 65_536 + tails[2], b"aaab" * 25_000]
    text, at, skip = filled([un_rle1(r) for r in rles])
    cut = pieces(text, [c for k, r in enumerate(rles) for c in (at[k], at[k] + len(un_rle1(r)))])
    blocks = [Block(p) if i % 2 == 0 else Block(rle=rles[i // 2]) for i, p in enumerate(cut)]
    assert all(blocks[2 * k + 1].text == cut[2 * k + 1] for k in range(4)) and blocks[1].n == blocks[7].n == 100_000
    add("long_runs", stream(blocks, level=1), text, skip,
        [f"run{d}:w{k}" for d in "ab" for k in range(16)] + ["n:level_limit", "run:ends_at_level_limit", "run:before_eob", "level:1"])
    # -- the end-of-block symbol first and 50th of its group; a run in front of the end of block (a run FIRST in a block needs
    #    the smallest rotation to follow the smallest byte: a block of one byte value, as in block_sizes and periods)
    found = {}
    for n in range(60, 400):
        b = Block(letters(n, 17))
        for key, hit in (("eob_first", len(b.syms) % 50 == 1), ("eob_50th", len(b.syms) % 50 == 0), ("run_last", b.syms[-2] <= 1)):
            if hit and key not in found:
                found[key] = n
    assert len(found) == 3, found
    text, at, skip = filled([letters(n, 17) for n in found.values()])
    cut = pieces(text, [c for k, n in enumerate(found.values()) for c in (at[k], at[k] + n)])
    add("eob_and_run_positions", stream([Block(p) for p in cut]), text, skip,
        ["eob:first_of_group", "eob:50th_of_group", "run:before_eob", "run:len:1", "run:len:2", "run:len:3"])
    assert tuple(out) == NAMES, list(out)
    return out


def INVALID(header: bytes, body: bytes):
    out = {}
    whole = header + body

    def one(change, level=9, text=whole, **kw):
        b = Block(text, **kw)
        change(b)
        return stream([b], level)

    def setter(**kw):
        return lambda b: [setattr(b, k, v) for k, v in kw.items()]

    out["randomised"] = (one(setter(randomised=1)), "randomised block")
    out["no_byte_in_use"] = (one(setter(used=[])), "no byte value in use")
    for k in (0, 1, 7):
        out[f"tables_{k}"] = (one(setter(n_tables_field=k)), "bad number of Huffman tables")
    out["selectors_0"] = (one(setter(n_sel=0)), "bad number of selectors")
    out["selector_past_the_tables"] = (one(setter(unary={1: 2})), "selector past the Huffman tables")
    out["start_length_0"] = (one(setter(starts={0: 0})), "bad Huffman code length")
    out["start_length_21"] = (one(setter(starts={1: 21})), "bad Huffman code length")

    def step(start, detour):
        def change(b):
            b.starts, b.detours = {0: start}, {(0, 0): detour}
        return change

    out["step_below_1"] = (one(step(1, [-1])), "bad Huffman code length")
    out["step_above_20"] = (one(step(20, [+1])), "bad Huffman code length")

    def no_code(b):   # (all codes 20 bits long: the set is far from complete, and twenty 1 bits are none of its codes)
        b.tables = [[20] * b.alpha for _ in b.tables]
        b.raw_symbol = {60: "1" * 20}
    out["no_code_of_an_incomplete_set"] = (one(no_code), "bad Huffman code")

    def fewer(b):
        b.n_sel = b.groups - 1
    out["symbols_beyond_the_selectors"] = (one(fewer), "selector past the Huffman tables")

    def digits(b):
        b.syms = b.syms[:10] + [0] * 21 + b.syms[10:]
        b.selectors = b.selectors + [0]
    out["run_digit_2_20"] = (one(digits), "bad run length")
    co = header + b"@CO\t"
    full = b"aaab" * 25_000
    out["n_above_the_level"] = (stream([Block(co), Block(full + b"c"), Block(b"\n" + body)], 1), "block longer than its stream's level allows")

    b = Block(full)   # (its last run, 74 999 bytes up to the block's 100 000th: one byte more)
    k = len(run_digits(74_999))
    assert b.syms[-1 - k:-1] == run_digits(74_999)
    b.syms[-1 - k:-1] = run_digits(75_000)
    out["run_overshoots"] = (stream([Block(co), b, Block(b"\n" + body)], 1), "block longer than its stream's level allows")

    def orig_n(b):
        b.orig = b.n
    out["orig_ptr_n"] = (one(orig_n), "origPtr out of range")

    def crc(b):
        b.crc ^= 0x100
    out["block_crc"] = (one(crc), "block CRC mismatch")
    good = stream([Block(whole)])
    out["combined_crc"] = (good[:-2] + bytes([good[-2] ^ 0x10]) + good[-1:], "combined CRC mismatch")
    # a block whose RLE1 string ends in four equal bytes and no count byte: bzip2 refuses it (its reader runs past the block's end)
    a = _a_runs(body)[0]
    cut = len(header) + a[0] + 4
    out["count_byte_missing"] = (stream([Block(text=whole[:cut], rle=rle1(whole[:cut])[:-1]), Block(whole[cut:])]), "bad run length")
    assert tuple(out) == INVALID_NAMES, list(out)
    return out
