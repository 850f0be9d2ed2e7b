"""A path-counting LZMA2 decoder in plain Python, written from the xz file format and the LZMA SDK's specification -- not
from slimm_amd/csrc/xz_stream.h --: the LZMA2 data of a block to its bytes and a Counter of the named paths the data took
(chunk controls, properties, literals per prior state, matches and reps per prior state, the length trees, distance slots,
the copy shapes, what a match reaches).  By it tests state which paths of the entropy decoder an input reaches; the container
around the data is tests/sam_xz.py's.  Slow (a few microseconds a bit); test infrastructure only."""
from collections import Counter

from tests import sam_xz as X

LEN_EDGES = (2, 9, 10, 17, 18, 273)   # the ends of the low, mid and high length trees
KINDS = ("lit", "match", "rep0", "rep1", "rep2", "rep3", "shortrep")


class Bad(Exception):
    pass


class _Rc:
    """The range decoder over b[p:end]."""
    def __init__(self, b, p, end):
        if end - p < 5 or b[p] != 0:
            raise Bad("range coder start")
        self.b, self.p, self.end = b, p + 5, end
        self.code, self.range = int.from_bytes(b[p + 1:p + 5], "big"), 0xFFFFFFFF

    def _norm(self):
        if self.range < 1 << 24:
            if self.p >= self.end:
                raise Bad("compressed bytes of the chunk used up")
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.code = ((self.code << 8) | self.b[self.p]) & 0xFFFFFFFF
            self.p += 1

    def bit(self, probs, i):
        self._norm()
        p = probs[i]
        bound = (self.range >> 11) * p
        if self.code < bound:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
            return 0
        self.range -= bound
        self.code -= bound
        probs[i] = p - (p >> 5)
        return 1

    def tree(self, probs, base, bits):
        m = 1
        for _ in range(bits):
            m = (m << 1) | self.bit(probs, base + m)
        return m - (1 << bits)

    def rtree(self, probs, base, bits):
        m, v = 1, 0
        for k in range(bits):
            bit = self.bit(probs, base + m)
            m = (m << 1) | bit
            v |= bit << k
        return v

    def direct(self, n):
        v = 0
        for _ in range(n):
            self._norm()
            self.range >>= 1
            bit = 1 if self.code >= self.range else 0
            if bit:
                self.code -= self.range
            v = (v << 1) | bit
        return v

    def finish(self):
        self._norm()
        if self.code != 0 or self.p != self.end:
            raise Bad("the chunk's compressed bytes do not end with its text")


class _Len:
    def __init__(self):
        self.choice = [1024, 1024]
        self.low = [1024] * (16 << 3)
        self.mid = [1024] * (16 << 3)
        self.high = [1024] * 256

    def decode(self, rc, ps):
        if not rc.bit(self.choice, 0):
            return 2 + rc.tree(self.low, ps << 3, 3), "low"
        if not rc.bit(self.choice, 1):
            return 10 + rc.tree(self.mid, ps << 3, 3), "mid"
        return 18 + rc.tree(self.high, 0, 8), "high"


class _State:
    """The probabilities, the state and the four distances: what a state reset renews."""
    def __init__(self, lc, lp, pb):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.lit = [1024] * (0x300 << (lc + lp))
        self.is_match = [1024] * (12 << 4)
        self.is_rep = [1024] * 12
        self.is_rep0 = [1024] * 12
        self.is_rep1 = [1024] * 12
        self.is_rep2 = [1024] * 12
        self.is_rep0_long = [1024] * (12 << 4)
        self.slot = [1024] * (4 << 6)
        self.special = [1024] * 128   # (the reverse trees of slots 4 .. 13, at base - slot - 1)
        self.align = [1024] * 16
        self.match_len, self.rep_len = _Len(), _Len()
        self.state, self.reps, self.fresh = 0, [0, 0, 0, 0], True


def props_of(byte):
    if byte > 224:
        raise Bad("properties byte above 224")
    lc, lp, pb = byte % 9, byte // 9 % 5, byte // 45
    if lc + lp > 4:
        raise Bad("lc + lp > 4")
    return lc, lp, pb


def decode_lzma2(b: bytes, p: int, dict_size: int):
    """The LZMA2 data at b[p]: (its bytes, the Counter of its paths, the offset behind its end marker)."""
    out, paths = bytearray(), Counter()
    st, props = None, None
    dict_from = None          # where the dictionary starts in `out`
    kinds = []                # per chunk so far: ("raw" | "lzma", its end in `out`)
    need_dict, need_props, need_state = True, True, True
    k = 0
    while True:
        c = b[p]
        if c == 0:
            return bytes(out), paths, p + 1
        where = "first" if k == 0 else "later"
        if c >= 0x80:
            usize, csize = (((c & 0x1f) << 16) | (b[p + 1] << 8) | b[p + 2]) + 1, ((b[p + 3] << 8) | b[p + 4]) + 1
            cls = c & 0xe0
            paths[f"control:{where}:0x{cls:02x}"] += 1
            if kinds:
                paths[f"control:0x{cls:02x}:after_{kinds[-1][0]}"] += 1
            p += 5
            if cls == 0xe0:
                dict_from, need_dict = len(out), False
            elif need_dict:
                raise Bad("no dictionary reset")
            if cls >= 0xc0:
                props = props_of(b[p])
                p += 1
                need_props = False
            elif need_props:
                raise Bad("no properties")
            if cls >= 0xa0:
                st = _State(*props)
                need_state = False
                paths["state_reset"] += 1
            elif need_state:
                raise Bad("no state reset")
            paths["props:lc%dlp%dpb%d" % props] += 1
            _chunk(b, p, p + csize, usize, out, dict_from, dict_size, st, kinds, paths)
            kinds.append(("lzma", len(out)))
            p += csize
        else:
            if c > 2:
                raise Bad("control byte 3 .. 0x7f")
            n = ((b[p + 1] << 8) | b[p + 2]) + 1
            paths[f"control:{where}:0x{c:02x}"] += 1
            if kinds:
                paths[f"control:0x{c:02x}:after_{kinds[-1][0]}"] += 1
            if c == 1:
                dict_from, need_dict = len(out), False
                need_props = True          # (a dictionary reset by an uncompressed chunk: the next LZMA chunk sets its properties anew)
                if k:
                    paths["raw_dict_reset_mid_block"] += 1
            elif need_dict:
                raise Bad("no dictionary reset")
            out += b[p + 3:p + 3 + n]
            if len(b) < p + 3 + n:
                raise Bad("truncated")
            kinds.append(("raw", len(out)))
            p += 3 + n
        k += 1


def _chunk(b, p, end, usize, out, dict_from, dict_size, s, kinds, paths):
    rc = _Rc(b, p, end)
    start, stop = len(out), len(out) + usize
    lc, lp, pb = s.lc, s.lp, s.pb
    pmask, lpmask = (1 << pb) - 1, (1 << lp) - 1
    reps = s.reps
    while len(out) < stop:
        n = len(out)
        at = n - dict_from      # (positions count from the dictionary's start)
        ps, state = at & pmask, s.state
        if not rc.bit(s.is_match, (state << 4) | ps):
            prev = out[n - 1] if n > dict_from else 0
            base = 0x300 * (((at & lpmask) << lc) | (prev >> (8 - lc)))
            sym = 1
            if state >= 7:
                mb = out[n - reps[0] - 1]
                agree = 0
                m = mb
                while sym < 0x100:
                    m <<= 1
                    mbit = m & 0x100
                    bit = rc.bit(s.lit, base + 0x100 + mbit + sym)
                    sym = (sym << 1) | bit
                    if mbit != bit << 8:
                        break
                    agree += 1
                while sym < 0x100:
                    sym = (sym << 1) | rc.bit(s.lit, base + sym)
                paths[f"lit:matched:s{state}"] += 1
                paths[f"lit:matched:agree{agree}"] += 1
            else:
                while sym < 0x100:
                    sym = (sym << 1) | rc.bit(s.lit, base + sym)
                paths[f"lit:plain:s{state}"] += 1
            out.append(sym & 0xff)
            if s.fresh:
                paths["fresh_reps:lit"] += 1
            s.state = 0 if state < 4 else state - 3 if state < 10 else state - 6
            continue
        if not rc.bit(s.is_rep, state):
            kind = "match"
            length, tree = s.match_len.decode(rc, ps)
            coder = "match"
            lstate = min(length - 2, 3)
            paths[f"lenstate:{lstate}"] += 1
            slot = rc.tree(s.slot, lstate << 6, 6)
            paths[f"slot:{slot}"] += 1
            if slot < 4:
                d = slot
            else:
                nb = (slot >> 1) - 1
                d = (2 | (slot & 1)) << nb
                if slot < 14:
                    d += rc.rtree(s.special, d - slot - 1, nb)
                else:
                    d += rc.direct(nb - 4) << 4
                    d += rc.rtree(s.align, 0, 4)
            if d == 0xFFFFFFFF:
                raise Bad("end marker inside an LZMA2 chunk")
            reps[3], reps[2], reps[1], reps[0] = reps[2], reps[1], reps[0], d
            s.state = 7 if state < 7 else 10
            fresh, s.fresh = False, False
        else:
            fresh = s.fresh
            if not rc.bit(s.is_rep0, state):
                if not rc.bit(s.is_rep0_long, (state << 4) | ps):
                    paths[f"shortrep:s{state}"] += 1
                    if fresh:
                        paths["fresh_reps:shortrep"] += 1
                    if n - dict_from <= reps[0]:
                        raise Bad("a distance beyond the bytes written")
                    if reps[0] >= dict_size:
                        raise Bad("a distance beyond the dictionary")
                    _reach(paths, n, reps[0], 1, start, kinds, dict_from, dict_size)
                    out.append(out[n - reps[0] - 1])
                    s.state = 9 if state < 7 else 11
                    continue
                kind = "rep0"
            else:
                if not rc.bit(s.is_rep1, state):
                    kind, d = "rep1", reps[1]
                else:
                    if not rc.bit(s.is_rep2, state):
                        kind, d = "rep2", reps[2]
                    else:
                        kind, d = "rep3", reps[3]
                        reps[3] = reps[2]
                    reps[2] = reps[1]
                reps[1] = reps[0]
                reps[0] = d
            length, tree = s.rep_len.decode(rc, ps)
            coder = "rep"
            s.state = 8 if state < 7 else 11
        paths[f"{kind}:s{state}"] += 1
        if fresh:
            paths[f"fresh_reps:{kind}"] += 1
        paths[f"len:{coder}:{tree}"] += 1
        if length in LEN_EDGES:
            paths[f"len:{coder}:{length}"] += 1
            paths[f"len:{coder}:{length}:pb{pb}:ps{ps}"] += 1
        d = reps[0]
        if n - dict_from <= d:
            raise Bad("a distance beyond the bytes written")
        if d >= dict_size:
            raise Bad("a distance beyond the dictionary")
        if n + length > stop:
            raise Bad("a match over the chunk's end")
        if n + length == stop:
            paths["match_ends_chunk"] += 1
        dist = d + 1
        if dist < length:
            paths["copy:dist<len"] += 1
        if dist < 8 and length >= 8:
            paths["copy:dist1-7,len>=8"] += 1
        if dist == 8:
            paths["copy:dist8"] += 1
        _reach(paths, n, d, length, start, kinds, dict_from, dict_size)
        if dist >= length:
            out += out[n - dist:n - dist + length]
        else:
            for _ in range(length):
                out.append(out[len(out) - dist])
    rc.finish()


def _reach(paths, n, d, length, start, kinds, dict_from, dict_size):
    """What a copy at `n` from distance d + 1 reaches."""
    src = n - d - 1
    if src < start:
        for kind, end in kinds:
            if end > src:
                paths[f"reach:earlier_{kind}_chunk"] += 1
                if kind == "raw" and d + 1 in (1, 7, 8, 9):
                    paths[f"reach:earlier_raw_chunk:dist{d + 1}"] += 1
                break
    if src == dict_from:
        paths["reach:first_byte_of_dictionary"] += 1
    if d + 1 == dict_size:
        paths["reach:dictionary_size"] += 1


def dict_size_of(byte: int) -> int:
    if byte > 40:
        raise Bad("dictionary size byte above 40")
    return 0xFFFFFFFF if byte == 40 else (2 | (byte & 1)) << (byte // 2 + 11)


def decode(blob: bytes):
    """Every stream of an xz file (LZMA2 alone in every block): (the text, the Counter of paths)."""
    text, paths = [], Counter()
    for s in X.walk(blob):
        for blk in s["blocks"]:
            assert [f for f, _ in blk["filters"]] == [0x21]
            out, c, end = decode_lzma2(blob, blk["data_at"], dict_size_of(blk["filters"][0][1][0]))
            assert end == blk["pad_at"]
            if X.CHECK_BYTES[s["check"]] and s["check"] != 10:
                if X.check_of(s["check"], out) != blob[blk["check_at"]:blk["check_at"] + X.CHECK_BYTES[s["check"]]]:
                    raise Bad("check mismatch")
            text.append(out)
            paths += c
    return b"".join(text), paths


def all_paths(max_slot=43, pbs=(4,)):
    """Every path name the decoder can count, the size-bounded ones included (slots up to 63)."""
    out = [f"control:first:0x{c:02x}" for c in (0x01, 0xe0)]
    out += [f"control:later:0x{c:02x}" for c in (0x01, 0x02, 0x80, 0xa0, 0xc0, 0xe0)]
    out += [f"control:0x{c:02x}:after_{k}" for c in (0x01, 0x02, 0x80, 0xa0, 0xc0, 0xe0) for k in ("raw", "lzma") if not (c == 0x80 and k == "raw")]
    out += ["state_reset", "raw_dict_reset_mid_block"]
    out += ["props:lc%dlp%dpb%d" % (lc, 4 - lc, pb) for lc in range(5) for pb in range(5)]
    out += [f"lit:plain:s{s}" for s in range(7)] + [f"lit:matched:s{s}" for s in range(7, 12)] + [f"lit:matched:agree{k}" for k in range(9)]
    out += [f"{k}:s{s}" for k in KINDS[1:] for s in range(12)]
    out += [f"fresh_reps:{k}" for k in ("lit", "rep0", "rep1", "rep2", "rep3", "shortrep")]
    for coder in ("match", "rep"):
        out += [f"len:{coder}:{t}" for t in ("low", "mid", "high")] + [f"len:{coder}:{v}" for v in LEN_EDGES]
        out += [f"len:{coder}:{v}:pb{pb}:ps{ps}" for v in LEN_EDGES for pb in pbs for ps in range(1 << pb)]
    out += [f"slot:{k}" for k in range(64)] + [f"lenstate:{k}" for k in range(4)]
    out += ["copy:dist<len", "copy:dist1-7,len>=8", "copy:dist8", "match_ends_chunk", "reach:earlier_lzma_chunk", "reach:earlier_raw_chunk"]
    out += [f"reach:earlier_raw_chunk:dist{d}" for d in (1, 7, 8, 9)] + ["reach:first_byte_of_dictionary", "reach:dictionary_size"]
    return out
