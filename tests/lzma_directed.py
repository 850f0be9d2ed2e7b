"""Directed xz inputs, written in plain Python and deterministic: a range encoder (adaptive bit, bit tree, reverse bit tree,
direct bits), an LZMA symbol encoder that takes the parse the test chooses -- literals, match(distance, length), rep(i, length),
short rep --, and an LZMA2 chunker with a chosen control byte per chunk.  tests/sam_xz.py's stream_of / block_header wrap the
data.  Any valid parse is a valid stream, so the only match finder is a small greedy one for the records behind the directed
part.  Every input decodes to a SAM text: its header, `@CO` lines that carry what SAM fields cannot (skipped with the header),
and a few records.  INPUTS() lists them, one path family each, with the paths of tests/lzma_paths.py each is named for.
Written from the LZMA SDK's specification; test infrastructure only."""
import random

from tests import sam_xz as X


class _Rc:
    def __init__(self):
        self.low, self.range, self.cache, self.pending, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def _shift(self):
        if self.low < 0xFF000000 or self.low >> 32:
            carry, b = self.low >> 32, self.cache
            while self.pending:
                self.out.append((b + carry) & 0xff)
                b = 0xff
                self.pending -= 1
            self.cache = (self.low >> 24) & 0xff
        self.pending += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, probs, i, bit):
        p = probs[i]
        bound = (self.range >> 11) * p
        if bit:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift()

    def tree(self, probs, base, bits, v):
        m = 1
        for k in range(bits - 1, -1, -1):
            b = (v >> k) & 1
            self.bit(probs, base + m, b)
            m = (m << 1) | b

    def rtree(self, probs, base, bits, v):
        m = 1
        for k in range(bits):
            b = (v >> k) & 1
            self.bit(probs, base + m, b)
            m = (m << 1) | b

    def direct(self, n, v):
        for k in range(n - 1, -1, -1):
            self.range >>= 1
            if (v >> k) & 1:
                self.low += self.range
            while self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self._shift()

    def finish(self) -> bytes:
        for _ in range(5):
            self._shift()
        return bytes(self.out)


class _Len:
    def __init__(self):
        self.choice, self.low, self.mid, self.high = [1024, 1024], [1024] * 128, [1024] * 128, [1024] * 256

    def encode(self, rc, ps, n):
        if n < 10:
            rc.bit(self.choice, 0, 0)
            rc.tree(self.low, ps << 3, 3, n - 2)
        elif n < 18:
            rc.bit(self.choice, 0, 1)
            rc.bit(self.choice, 1, 0)
            rc.tree(self.mid, ps << 3, 3, n - 10)
        else:
            rc.bit(self.choice, 0, 1)
            rc.bit(self.choice, 1, 1)
            rc.tree(self.high, 0, 8, n - 18)


class _Model:
    def __init__(self, lc, lp, pb):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.lit = [1024] * (0x300 << (lc + lp))
        self.is_match, self.is_rep0_long = [1024] * 192, [1024] * 192
        self.is_rep, self.is_rep0, self.is_rep1, self.is_rep2 = [1024] * 12, [1024] * 12, [1024] * 12, [1024] * 12
        self.slot, self.special, self.align = [1024] * 256, [1024] * 128, [1024] * 16
        self.match_len, self.rep_len = _Len(), _Len()
        self.state, self.reps = 0, [0, 0, 0, 0]


def lit(data: bytes):
    return ("lit", bytes(data))


def match(dist: int, length: int):
    return ("match", dist, length)


def rep(i: int, length: int):
    return ("rep", i, length)


SHORTREP = ("shortrep",)


class Lzma2:
    """The LZMA2 data of one block, chunk by chunk; `text` grows with it.  valid=False: a parse may leave the format (for the
    invalid variants) -- distances and lengths are then not checked against the text."""
    def __init__(self, dict_size=1 << 16, valid=True):
        self.text, self.chunks, self.dict_from, self.dict_size, self.valid = bytearray(), [], 0, dict_size, valid
        self.model, self.props = None, (3, 0, 2)

    def raw(self, data: bytes, control=2):
        assert 1 <= len(data) <= 1 << 16
        if control == 1:
            self.dict_from = len(self.text)
        self.chunks.append(bytes([control, (len(data) - 1) >> 8, (len(data) - 1) & 0xff]) + data)
        self.text += data
        return self

    def filler(self, n: int, seed: int):
        """n bytes of seeded filler (no tab, no newline) in uncompressed chunks of control 2."""
        rng = random.Random(seed)
        data = bytes(rng.choice(b"ACGTacgtNn0123456789!#$%&()*+,-./:;<=>?") for _ in range(min(n, 4099)))
        data = (data * (n // len(data) + 1))[:n]
        for i in range(0, n, 1 << 16):
            self.raw(data[i:i + (1 << 16)])
        return self

    def lzma(self, ops, control=0x80, props=None, usize=None):
        """One LZMA chunk of the parse `ops`; control 0x80 / 0xa0 / 0xc0 / 0xe0; props (lc, lp, pb) with 0xc0 and 0xe0.
        usize: what the header states when not the parse's (invalid variants)."""
        if control >= 0xc0:
            self.props = props or self.props
        if control == 0xe0:
            self.dict_from = len(self.text)
        if control >= 0xa0:
            self.model = _Model(*self.props)
        m, rc, t, start = self.model, _Rc(), self.text, len(self.text)
        pmask, lpmask = (1 << m.pb) - 1, (1 << m.lp) - 1
        for op in ops:
            if op[0] == "lit":
                for byte in op[1]:
                    at = len(t) - self.dict_from
                    rc.bit(m.is_match, (m.state << 4) | (at & pmask), 0)
                    prev = t[-1] if at else 0
                    base = 0x300 * (((at & lpmask) << m.lc) | (prev >> (8 - m.lc)))
                    sym = 1
                    if m.state >= 7:
                        mb, offs = t[len(t) - m.reps[0] - 1], 0x100
                        for k in range(7, -1, -1):
                            mb <<= 1
                            mbit, b = mb & offs, (byte >> k) & 1
                            rc.bit(m.lit, base + offs + mbit + sym, b)
                            sym = (sym << 1) | b
                            if mbit != b << 8:
                                offs = 0
                    else:
                        for k in range(7, -1, -1):
                            b = (byte >> k) & 1
                            rc.bit(m.lit, base + sym, b)
                            sym = (sym << 1) | b
                    t.append(byte)
                    m.state = 0 if m.state < 4 else m.state - 3 if m.state < 10 else m.state - 6
                continue
            at = len(t) - self.dict_from
            ps, st = at & pmask, m.state
            rc.bit(m.is_match, (st << 4) | ps, 1)
            if op[0] == "match":
                _, dist, n = op
                rc.bit(m.is_rep, st, 0)
                m.match_len.encode(rc, ps, n)
                d = dist - 1
                if d < 4:
                    slot = d
                else:
                    nb = d.bit_length() - 1
                    slot = 2 * nb + ((d >> (nb - 1)) & 1)
                rc.tree(m.slot, min(n - 2, 3) << 6, 6, slot)
                if slot >= 4:
                    fb = (slot >> 1) - 1
                    base = (2 | (slot & 1)) << fb
                    if slot < 14:
                        rc.rtree(m.special, base - slot - 1, fb, d - base)
                    else:
                        rc.direct(fb - 4, (d - base) >> 4)
                        rc.rtree(m.align, 0, 4, (d - base) & 15)
                m.reps = [d] + m.reps[:3]
                m.state = 7 if st < 7 else 10
            elif op[0] == "shortrep":
                rc.bit(m.is_rep, st, 1)
                rc.bit(m.is_rep0, st, 0)
                rc.bit(m.is_rep0_long, (st << 4) | ps, 0)
                m.state = 9 if st < 7 else 11
                n = 1
            else:
                _, i, n = op
                rc.bit(m.is_rep, st, 1)
                if i == 0:
                    rc.bit(m.is_rep0, st, 0)
                    rc.bit(m.is_rep0_long, (st << 4) | ps, 1)
                else:
                    rc.bit(m.is_rep0, st, 1)
                    rc.bit(m.is_rep1, st, int(i > 1))
                    if i > 1:
                        rc.bit(m.is_rep2, st, int(i > 2))
                    m.reps.insert(0, m.reps.pop(i))
                m.rep_len.encode(rc, ps, n)
                m.state = 8 if st < 7 else 11
            dist = m.reps[0] + 1
            if self.valid:
                assert dist <= at and dist <= self.dict_size, (op, at)
            elif dist > len(t):
                t += bytes(n)   # (what a decoder must refuse: the text behind it does not matter)
                continue
            for _ in range(n):
                t.append(t[len(t) - dist])
        data = rc.finish()
        n = (usize if usize is not None else len(t) - start) - 1
        assert 0 <= n < 1 << 21 and 1 <= len(data) <= 1 << 16, (n, len(data))
        head = bytes([control | (n >> 16), (n >> 8) & 0xff, n & 0xff, (len(data) - 1) >> 8, (len(data) - 1) & 0xff])
        if control >= 0xc0:
            lc, lp, pb = self.props
            head += bytes([(pb * 5 + lp) * 9 + lc])
        self.chunks.append(head + data)
        return self

    def data(self) -> bytes:
        return b"".join(self.chunks) + b"\x00"


def greedy(history: bytes, new: bytes, window: int, min_len=3, max_len=273):
    """A parse of `new` behind `history`: the longest of the last few earlier places with the same three bytes, else a literal."""
    t = bytes(history) + new
    seen, ops, p, lits = {}, [], len(history), bytearray()
    for i in range(max(0, len(history) - window), len(history) - 2):
        seen.setdefault(t[i:i + 3], []).append(i)
    while p < len(t):
        best, at = 0, 0
        for q in reversed(seen.get(t[p:p + 3], [])[-6:]):
            if p - q > window:
                break
            n = 0
            while p + n < len(t) and n < max_len and t[q + n] == t[p + n]:
                n += 1
            if n > best:
                best, at = n, q
        step = best if best >= min_len else 1
        if best >= min_len:
            if lits:
                ops.append(lit(lits))
                lits = bytearray()
            ops.append(match(p - at, best))
        else:
            lits.append(t[p])
        for i in range(p, min(p + step, len(t) - 2)):
            seen.setdefault(t[i:i + 3], []).append(i)
        p += step
    if lits:
        ops.append(lit(lits))
    return ops


def dict_byte_of(size: int) -> int:
    for b in range(41):
        if (2 | (b & 1)) << (b // 2 + 11) >= size:
            return b
    raise AssertionError(size)


NAMES = ("controls", "props_every_pb_and_split", "raw_lzma_raw_lzma", "raw_dict_reset_then_e0", "raw_dict_reset_then_c0", "length_edges_match",
         "length_edges_rep", "distance_slots", "reps_from_every_state", "matched_literals", "match_ends_chunk", "dict_4k_edges", "check_none",
         "two_blocks")
HISTORY = ("two_blocks",)      # (pushed with a round a block too: its force key)
INVALID_NAMES = ("distance_one_beyond_the_bytes_written", "distance_one_beyond_the_dictionary", "match_over_the_chunks_end",
                 "control_0x80_behind_a_raw_chunk", "control_0xa0_behind_a_dictionary_reset", "short_rep_into_an_empty_dictionary")


# ---- the inputs -----------------------------------------------------------------------------------------------------------
def _line(payload: bytes) -> bytes:
    return b"@CO\t" + payload + b"\n"


def _letters(n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGTNacgtn !#0123456789:;<=>?IJKLMNOPQRST~") for _ in range(n))


class _Input:
    """One block: the header in a first chunk, the directed chunks (`@CO` lines), the records in the last chunks."""
    def __init__(self, header: bytes, records: bytes, dict_size=1 << 16, check=4, first=0xe0, props=(3, 0, 2)):
        self.z, self.records, self.check, self.header = Lzma2(dict_size), records, check, header
        if first == 1:
            self.z.raw(header, control=1)
        else:
            self.z.lzma(greedy(b"", header, dict_size), 0xe0, props)

    def done(self, control=0x80, props=None):
        z = self.z
        skip = len(z.text)
        assert z.text[:len(self.header)] == self.header and z.text.endswith(b"\n")
        z.lzma(greedy(z.text[z.dict_from:], self.records, min(z.dict_size, 1 << 15)), control, props)
        text = bytes(z.text)
        blob = X.stream_of([(X.block_header(dict_byte_of(z.dict_size)), z.data(), text)], self.check)
        return blob, text, skip


def _co(z, ops, control=0x80, props=None):
    """A chunk that is one `@CO` line: the line's start and its newline as literals around `ops`."""
    return z.lzma([lit(b"@CO\t")] + ops + [lit(b"\n")], control, props)


def INPUTS(header: bytes, records: bytes):
    """{name: (xz bytes, text, skip, [paths it is named for], the force key by which a history case is pushed once more, a round a
    block, or None)}."""
    out = {}

    def add(name, inp, paths, done=None, force=None):
        blob, text, skip = inp.done(**(done or {}))
        out[name] = (blob, text, skip, paths, force)

    def new(**kw):
        return _Input(header, records, **kw)

    # -- the four LZMA controls in later position; 0xc0 changes lc / lp / pb mid-block
    i = new()
    for k, (c, pr) in enumerate([(0x80, None), (0xa0, None), (0xc0, (1, 2, 3)), (0x80, None), (0xa0, None), (0xe0, (0, 4, 0)), (0xc0, (4, 0, 1))]):
        line = _line(_letters(150, k) + _letters(40, k) * 3)
        i.z.lzma(greedy(i.z.text[i.z.dict_from:] if c != 0xe0 else b"", line, 1 << 15), c, pr)
    add("controls", i, [f"control:later:0x{c:02x}" for c in (0x80, 0xa0, 0xc0, 0xe0)] + ["props:lc0lp4pb0", "props:lc4lp0pb1"],
        done=dict(control=0xa0))
    # -- every pb with every legal lc + lp = 4 split, set by 0xc0
    i = new(check=1)
    for k, (lc, pb) in enumerate((lc, pb) for lc in range(5) for pb in range(5)):
        line = _line(_letters(90, 100 + k) + _letters(23, k) * 2)
        i.z.lzma(greedy(i.z.text, line, 1 << 15), 0xc0, (lc, 4 - lc, pb))
    add("props_every_pb_and_split", i, ["props:lc%dlp%dpb%d" % (lc, 4 - lc, pb) for lc in range(5) for pb in range(5)], done=dict(control=0xc0, props=(3, 0, 2)))
    # -- raw -> LZMA -> raw -> LZMA: matches from the LZMA chunks into the raw bytes at distance 1, 7, 8, 9 and the largest
    i = new(first=1, dict_size=1 << 16)
    z = i.z
    _co(z, [match(len(z.text) + 4, 30), lit(b"x")], 0xc0, (3, 0, 2))          # (the largest: back to the block's first byte)
    z.raw(b"@CO\t" + _letters(60, 5))
    z.lzma([match(1, 2), match(7, 2), match(8, 2), match(9, 3), lit(b"|")], 0xa0)      # (short copies, each from the raw bytes)
    for k, d in enumerate((1, 7, 8, 9)):                                                 # (long ones that run on into their own bytes)
        z.raw(_letters(11, 50 + k))
        z.lzma([match(d, 12 + k), lit(b"|")], 0xa0 if k % 2 else 0xc0, (3, 0, 2))
    z.raw(b"\n")
    add("raw_lzma_raw_lzma", i, ["control:0xa0:after_raw", "control:0x02:after_lzma", "control:0xc0:after_raw", "reach:earlier_raw_chunk",
                                 "reach:first_byte_of_dictionary"] + [f"reach:earlier_raw_chunk:dist{d}" for d in (1, 7, 8, 9)], done=dict(control=0xa0))
    # -- an uncompressed chunk that resets the dictionary mid-block, then 0xe0; and then 0xc0 only
    for name, c in (("raw_dict_reset_then_e0", 0xe0), ("raw_dict_reset_then_c0", 0xc0)):
        i = new(check=1)
        z = i.z
        _co(z, [lit(_letters(33, 7)), match(20, 40)])      # (an odd length: the positions behind the reset start at 0 again)
        z.raw(_line(_letters(45, 8)), control=1)
        line = [lit(b"@CO\t"), match(len(z.text) - z.dict_from + 4, 40), lit(_letters(20, 9)), rep(0, 9), lit(b"\n")]
        if c == 0xe0:
            z.raw(_line(b"dropped with the next reset"), control=1)
            line[1] = lit(b"a new dictionary")
        z.lzma(line, c, (2, 1, 3))
        add(name, i, ["raw_dict_reset_mid_block", f"control:0x{c:02x}:after_raw", "control:0x01:after_lzma"] + (["reach:first_byte_of_dictionary"] if c == 0xc0 else []))
    # -- the length trees' ends in both coders, at every pos_state of pb = 4
    for coder in ("match", "rep"):
        i = new(props=(0, 4, 4) if coder == "rep" else (3, 0, 4))
        z = i.z
        base = _letters(300, 11)
        z.lzma([lit(b"@CO\t" + base)], 0x80)
        for n in (2, 9, 10, 17, 18, 273):
            ops = []
            for ps in range(16):
                while (len(z.text) - z.dict_from + sum(len(o[1]) if o[0] == "lit" else o[2] for o in ops)) % 16 != ps:
                    ops.append(lit(b"."))
                d = len(z.text) + sum(len(o[1]) if o[0] == "lit" else o[2] for o in ops) - len(header) - 4
                ops += [match(d, n)] if coder == "match" else [match(d, 3), lit(b",,"), rep(0, n)]
                ops.append(lit(b";"))
            z.lzma(ops, 0x80)
        z.lzma([lit(b"\n")], 0x80)
        add(f"length_edges_{coder}", i, [f"len:{coder}:{n}:pb4:ps{ps}" for n in (2, 9, 10, 17, 18, 273) for ps in range(16)]
            + [f"len:{coder}:{t}" for t in ("low", "mid", "high")] + [f"len:{coder}:273"])
    # -- every distance slot a 4 MiB dictionary allows, the far ones over uncompressed filler
    i = new(dict_size=1 << 22, check=1)
    z = i.z
    z.lzma([lit(b"@CO\t")], 0x80)
    z.filler((1 << 22) - len(z.text) - 600, 13)
    ops = [lit(b"slots:")]
    for slot in range(44):
        d = slot if slot < 4 else (2 | (slot & 1)) << ((slot >> 1) - 1)
        ops += [match(d + 1, 2 + slot % 4), lit(b"/")]                       # (the slot's first distance ...)
        if slot >= 4 and slot < 43:
            ops += [match(((3 + (slot & 1)) << ((slot >> 1) - 1)), 5), lit(b"\\")]   # (... and its last)
    z.lzma(ops, 0xa0)
    pad = (1 << 22) - len(z.text)
    z.lzma([lit(b"=" * pad), match(1 << 22, 7), lit(b"\n")], 0x80)
    add("distance_slots", i, [f"slot:{k}" for k in range(44)] + [f"lenstate:{k}" for k in range(4)] + ["reach:dictionary_size"])
    # -- rep0 .. rep3 and short rep from every state; and right behind a state reset, where all four distances are 0
    i = new()
    z = i.z
    tail = {0: [lit(b"ab")], 7: [match(9, 2)], 8: [lit(b"x"), rep(1, 3)], 9: [lit(b"y"), SHORTREP], 10: [match(5, 2), match(11, 3)], 11: [match(5, 2), rep(1, 2)]}
    for st in (1, 2, 3, 4, 5, 6):   # (the literal states: so many literals behind a match, rep or short rep)
        tail[st] = {4: tail[7] + [lit(b"q")], 5: tail[8] + [lit(b"r")], 6: tail[9] + [lit(b"s")], 1: tail[7] + [lit(b"tu")], 2: tail[8] + [lit(b"vw")],
                    3: tail[9] + [lit(b"zz")]}[st]
    kinds = [("match", lambda: match(13, 4)), ("rep0", lambda: rep(0, 3)), ("rep1", lambda: rep(1, 3)), ("rep2", lambda: rep(2, 3)),
             ("rep3", lambda: rep(3, 3)), ("shortrep", lambda: SHORTREP), ("lit", lambda: lit(b"L"))]
    z.lzma([lit(b"@CO\t" + _letters(64, 17))], 0x80)
    for st in range(12):
        for kind, op in kinds:
            # four distinct distances first, then the state, then the symbol; then every distance read back, the last one first
            probe = [lit(b"."), rep(3, 2), lit(b","), rep(3, 3), lit(b","), rep(3, 2), lit(b","), rep(3, 3), lit(b".")]
            z.lzma([match(17, 2), lit(b"-"), match(19, 2), lit(b"-"), match(23, 2), lit(b"-"), match(29, 2), lit(b"-")] + tail[st] + [op()] + probe, 0x80)
    z.lzma([lit(b"\n")], 0x80)
    for k, kind in enumerate(("rep0", "rep1", "rep2", "rep3", "shortrep", "lit")):
        first = {"lit": lit(b"@"), "shortrep": SHORTREP}.get(kind) or rep(int(kind[3]), 4)
        line = _line(_letters(12, 20 + k) + b"@@@@@")[:-1]
        if k % 2:
            z.raw(line)
        else:
            z.lzma([lit(line)], 0xa0)
        z.lzma([first, lit(b"\n")], 0xa0)
    add("reps_from_every_state", i, [f"{k}:s{s}" for k in ("match", "rep0", "rep1", "rep2", "rep3", "shortrep") for s in range(12)]
        + [f"lit:plain:s{s}" for s in range(7)] + [f"lit:matched:s{s}" for s in range(7, 12)]
        + [f"fresh_reps:{k}" for k in ("lit", "rep0", "rep1", "rep2", "rep3", "shortrep")], done=dict(control=0xa0))
    # -- the matched literal: the byte at the last distance agrees with it in 0 .. 8 leading bits
    i = new(check=1)
    z = i.z
    ops = [lit(b"@CO\t" + b"U" * 40)]       # (0x55)
    for agree in range(9):
        byte = 0x55 if agree == 8 else 0x55 ^ (0x80 >> agree)
        for behind in ([match(3, 4)], [rep(0, 2)], [SHORTREP], [match(3, 2), match(5, 2)], [match(3, 2), rep(0, 2)]):
            ops += behind + [lit(bytes([byte])), lit(b"U" * 8)]
    z.lzma(ops, 0x80)
    z.lzma([lit(b"\n")], 0x80)
    text = bytes(z.text)
    assert b"\n" not in text[len(header):-1]
    add("matched_literals", i, [f"lit:matched:agree{k}" for k in range(9)] + [f"lit:matched:s{s}" for s in range(7, 12)])
    # -- a match that ends exactly with its chunk; copies that overlap themselves
    i = new()
    z = i.z
    z.lzma([lit(b"@CO\t" + _letters(20, 31)), match(1, 273)], 0x80)
    z.lzma([match(3, 100), lit(b"abcdefgh"), match(8, 64), match(7, 8), lit(b"\n"), match(4 + 20 + 273 + 100 + 8 + 64 + 8 + 1, 4)], 0x80)
    z.lzma([rep(0, 11), lit(b"\n")], 0x80)
    add("match_ends_chunk", i, ["match_ends_chunk", "copy:dist<len", "copy:dist1-7,len>=8", "copy:dist8", "reach:earlier_lzma_chunk"])
    # -- the smallest dictionary: a distance equal to the bytes written so far, and equal to the dictionary's 4 KiB
    i = new(dict_size=4096, check=1)
    z = i.z
    z.lzma([lit(b"@CO\t" + _letters(12, 36)), match(16, 16), lit(_letters(4096 - 32, 37)), match(4096, 30), lit(b"\n")], 0xe0, (3, 0, 2))
    add("dict_4k_edges", i, ["reach:first_byte_of_dictionary", "reach:dictionary_size"])
    # -- the no-check path only
    i = new(check=0)
    _co(i.z, [lit(_letters(50, 41)), match(25, 30)])
    add("check_none", i, [])
    # -- two blocks, for a round a block: the second block's dictionary starts with it, and its first match reaches its first byte
    a, b = Lzma2(), Lzma2()
    a.lzma(greedy(b"", header, 1 << 15) + [lit(b"@CO\t" + _letters(40, 43)), match(len(header) + 44, 12), lit(b"\n")], 0xe0, (3, 0, 2))
    b.lzma([lit(b"@CO\t" + _letters(40, 44)), match(44, 12), lit(b"\n")], 0xe0, (3, 0, 2))
    skip = len(a.text) + len(b.text)
    b.lzma(greedy(bytes(b.text), records, 1 << 15), 0x80)
    blob = X.stream_of([(X.block_header(dict_byte_of(z.dict_size)), z.data(), bytes(z.text)) for z in (a, b)], 4)
    out["two_blocks"] = (blob, bytes(a.text + b.text), skip, ["reach:first_byte_of_dictionary", "control:later:0x80"], "xz_round_text=1,xz_round=1")
    assert tuple(out) == NAMES, list(out)
    return out


def INVALID(header: bytes, records: bytes):
    """{name: (xz bytes, the decoder's words)}: what a decoder must refuse, each one rule broken in an otherwise good block."""
    out = {}

    def block(z, text=None):
        return X.stream_of([(X.block_header(dict_byte_of(z.dict_size)), z.data(), bytes(z.text) if text is None else text)], 4)

    def start(dict_size=1 << 16):
        z = Lzma2(dict_size, valid=False)
        z.lzma(greedy(b"", header, 1 << 15), 0xe0, (3, 0, 2))
        return z

    z = start()
    z.lzma([lit(b"@CO\t"), match(len(z.text) + 5, 4), lit(b"\n")], 0x80)
    out["distance_one_beyond_the_bytes_written"] = (block(z), "a distance beyond the block's start or dictionary")
    z = start(4096)
    z.lzma([lit(b"@CO\t" + _letters(4200, 3)), match(4097, 4), lit(b"\n")], 0x80)
    out["distance_one_beyond_the_dictionary"] = (block(z), "a distance beyond the block's start or dictionary")
    z = start()
    z.lzma([lit(b"@CO\t"), match(3, 20)], 0x80, usize=4 + 19)
    z.lzma([lit(b"\n")], 0x80)
    out["match_over_the_chunks_end"] = (block(z), "a match that runs over its chunk's end")
    z = start()
    z.raw(_line(b"uncompressed"))
    z.lzma([lit(_line(b"no state reset"))], 0x80)
    out["control_0x80_behind_a_raw_chunk"] = (block(z), "an LZMA chunk behind an uncompressed chunk does not reset the state")
    z = start()
    z.raw(_line(b"uncompressed, a new dictionary"), control=1)
    z.lzma([lit(_line(b"no properties"))], 0xa0)
    out["control_0xa0_behind_a_dictionary_reset"] = (block(z), "an LZMA chunk without properties in front of it")
    z = start()
    z.lzma([SHORTREP], 0xe0, (3, 0, 2))
    out["short_rep_into_an_empty_dictionary"] = (block(z), "a distance beyond the block's start or dictionary")
    assert tuple(out) == INVALID_NAMES
    return out
