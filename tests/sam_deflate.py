"""gzip copies of a SAM text whose deflate streams hold what the device inflater must handle -- many dynamic blocks, fixed
blocks, stored blocks, flushes, several members --, made with zlib under chosen settings; a pure-Python walker of deflate
blocks, by which tests state what their inputs contain; and a hand encoder of fixed-Huffman blocks and gzip framing for
streams zlib does not write.  Test infrastructure only."""
import struct
import zlib

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY,
              "filtered": zlib.Z_FILTERED}


def raw_deflate(text: bytes, level=6, memLevel=8, strategy="default", flush_every=0, flush=zlib.Z_SYNC_FLUSH, final=True) -> bytes:
    """`text` as a raw deflate stream (no framing); flush_every > 0: a flush of kind `flush` behind every so many bytes;
    final=False: ended by a Z_FULL_FLUSH instead of a final block (byte-aligned: pieces of this kind can be concatenated)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, memLevel, STRATEGIES[strategy])
    out = []
    step = flush_every or max(1, len(text))
    for i in range(0, len(text), step):
        out.append(c.compress(text[i:i + step]))
        if flush_every and i + step < len(text):
            out.append(c.flush(flush))
    out.append(c.flush(zlib.Z_FINISH if final else zlib.Z_FULL_FLUSH))
    return b"".join(out)


def gzip_frame(deflate: bytes, text: bytes, extra: bytes = None, name: bytes = None, comment: bytes = None, hcrc=False,
               crc=None, isize=None) -> bytes:
    """One gzip member around a raw deflate stream of `text`; the header fields as given; crc / isize: wrong ones on purpose."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h + deflate + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) & 0xffffffff) if isize is None else isize)


def member(text: bytes, **kw) -> bytes:
    frame = {k: kw.pop(k) for k in ("extra", "name", "comment", "hcrc", "crc", "isize") if k in kw}
    return gzip_frame(raw_deflate(text, **kw), text, **frame)


KINDS = {
    "default": dict(),
    "mem1": dict(memLevel=1),
    "mem3": dict(memLevel=3),
    "fixed": dict(strategy="fixed", memLevel=1),
    "rle": dict(strategy="rle", memLevel=2),
    "huffman": dict(strategy="huffman", memLevel=4),
    "sync": dict(flush_every=20_000),
    "stored": dict(level=0),
}


def three_members(text: bytes) -> bytes:
    """Members of different kinds back to back, an empty one among them, every header field in use somewhere."""
    a, b = len(text) // 3, 2 * len(text) // 3
    return (member(text[:a], memLevel=1, name=b"x.sam") + member(b"", comment=b"nothing here") +
            member(text[a:b], strategy="fixed", memLevel=1, extra=b"AB\x02\0hi", hcrc=True) + member(text[b:], flush_every=20_000))


def copy_of(text: bytes, kind: str) -> bytes:
    return three_members(text) if kind == "members" else member(text, **KINDS[kind])


# ---- a walker of deflate blocks ------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, bit=0):
        self.d, self.p = data, bit

    def get(self, k):
        v = 0
        for i in range(k):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def _huff(lengths):
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    offs = [0] * 16
    for n in range(1, 15):
        offs[n + 1] = offs[n] + count[n]
    sym = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            sym[offs[n]] = s
            offs[n] += 1
    return count, sym


def _decode(b, h):
    count, sym = h
    code = first = index = 0
    for n in range(1, 16):
        code |= b.get(1)
        if code - count[n] < first:
            return sym[index + code - first]
        index += count[n]
        first = (first + count[n]) << 1
        code <<= 1
    raise ValueError("bad code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
          12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_FIXED = (_huff([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _huff([5] * 30))


def blocks(deflate: bytes, bit: int = 0):
    """The blocks of a raw deflate stream from bit offset `bit` on: [(bit offset, type 0 / 1 / 2, final, text bytes)];
    and the bit behind the final block."""
    b = _Bits(deflate, bit)
    out = []
    while True:
        at = b.p
        final, typ = b.get(1), b.get(2)
        n = 0
        if typ == 0:
            b.p = (b.p + 7) & ~7
            n = b.get(16)
            assert b.get(16) == n ^ 0xffff
            b.p += 8 * n
        else:
            if typ == 1:
                lit, dist = _FIXED
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = b.get(3)
                ch, lens = _huff(cl), []
                while len(lens) < hlit + hdist:
                    s = _decode(b, ch)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    elif s == 17:
                        lens += [0] * (3 + b.get(3))
                    else:
                        lens += [0] * (11 + b.get(7))
                lit, dist = _huff(lens[:hlit]), _huff(lens[hlit:])
            while True:
                s = _decode(b, lit)
                if s < 256:
                    n += 1
                elif s == 256:
                    break
                else:
                    n += _LBASE[s - 257] + b.get(_LEXT[s - 257])
                    d = _decode(b, dist)
                    b.get(_DEXT[d])
        out.append((at, typ, bool(final), n))
        if final:
            return out, b.p


def member_blocks(blob: bytes):
    """blocks() of a one-member gzip file without optional header fields."""
    assert blob[:3] == b"\x1f\x8b\x08" and blob[3] == 0
    return blocks(blob[10:])[0]


def count_types(bl):
    return {t: sum(1 for b in bl if b[1] == t) for t in (0, 1, 2)}


# ---- a hand encoder of fixed-Huffman blocks ------------------------------------------------------------------------------
class FixedBlocks:
    """Raw deflate written symbol by symbol with the fixed codes: begin(final), literal / literals, match(length, distance),
    end(); align() writes an empty stored block, which ends on a byte, finish() pads the last byte behind a final block.
    bytes() gives the stream so far."""

    def __init__(self):
        self.acc = self.n = 0
        self.out = bytearray()

    def _put(self, v, k):   # k bits of v, the lowest first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def _code(self, v, k):   # a Huffman code: its highest bit first
        self._put(int(format(v, "0%db" % k)[::-1], 2), k)

    def _sym(self, s):
        if s < 144:
            self._code(0x30 + s, 8)
        elif s < 256:
            self._code(0x190 + s - 144, 9)
        elif s < 280:
            self._code(s - 256, 7)
        else:
            self._code(0xc0 + s - 280, 8)

    def begin(self, final=False):
        self._put(1 if final else 0, 1)
        self._put(1, 2)
        return self

    def literal(self, v):
        self._sym(v)
        return self

    def literals(self, data: bytes):
        for v in data:
            self._sym(v)
        return self

    def match(self, length, distance):
        i = 28 if length == 258 else max(k for k in range(28) if _LBASE[k] <= length)
        self._sym(257 + i)
        self._put(length - _LBASE[i], _LEXT[i])
        j = max(k for k in range(30) if _DBASE[k] <= distance)
        self._code(j, 5)
        self._put(distance - _DBASE[j], _DEXT[j])
        return self

    def end(self):
        self._sym(256)
        return self

    def align(self, final=False):
        self._put(1 if final else 0, 1)
        self._put(0, 2)
        if self.n:
            self._put(0, 8 - self.n)
        self.out += b"\0\0\xff\xff"
        return self

    def finish(self):   # behind a final block: the rest of its last byte
        if self.n:
            self._put(0, 8 - self.n)
        return self

    def bytes(self):
        assert self.n == 0, "align() or finish() first"
        return bytes(self.out)


# ---- crafted members: copies that reach in front of a chunk --------------------------------------------------------------
def _lines(body: bytes):
    out, p = [], 0
    while p < len(body):
        q = body.index(b"\n", p) + 1
        out.append(body[p:q])
        p = q
    return out


def _tiny_dynamic(text: bytes) -> bytes:
    """`text` as one non-final dynamic block and an empty stored block (a fresh compressor: it copies from nothing in front;
    Huffman codes only, so that the dynamic codes are worth their header)."""
    piece = raw_deflate(text, strategy="huffman", final=False)
    bl = blocks(piece + FixedBlocks().begin(True).end().finish().bytes())[0]
    assert [b[1] for b in bl[:2]] == [2, 0] and bl[0][3] == len(text), bl
    return piece


def far_copy_member(body: bytes, ref_name: bytes):
    """(gzip member, its text, compressed bytes in front of the crafted chunk).  The chunk starts with a tiny dynamic block
    and goes on, in a fixed block, with a copy of 258 + 254 bytes at distance 32 768 -- the farthest byte of the chunk in
    front -- and a run written as one byte and a copy at distance 1 of length 258.  The text stays whole SAM lines: some
    lines a second time, and a line whose SEQ is the run."""
    lines = _lines(body)
    # P: lines up to 40 000 bytes, padded by an optional field so that a line starts 32 768 bytes before its end
    P, k = b"", 0
    while len(P) < 40_000:
        P += lines[k]
        k += 1
    starts, p = [], 0
    for ln in lines[:k]:
        starts.append(p)
        p += len(ln)
    a = max(s for s in starts if len(P) - s >= 32_768 - 4_000 and len(P) - s <= 32_768 - 7)
    pad = 32_768 - (len(P) - a)
    i = starts.index(a)
    P = P[:a] + lines[i][:-1] + b"\tXX:Z:" + b"x" * (pad - 6) + b"\n" + P[a + len(lines[i]):]
    assert len(P) - a == 32_768
    # the chunk: D = P[a:s] as a dynamic block, then P[s:s + 512] copied, the rest of that line as literals
    s = a + 2_000
    b = P.index(b"\n", s + 512) + 1
    run_line = b"zrun\t0\t" + ref_name + b"\t1\t0\t*\t*\t0\t0\tA"
    f = FixedBlocks().begin().match(258, 32_768).match(254, 32_768).literals(P[s + 512:b]).literals(run_line).match(258, 1)
    f.literals(b"\t*\n").end().begin(True).end().finish()
    text = P + P[a:b] + run_line + b"A" * 258 + b"\t*\n"
    first = raw_deflate(P, memLevel=8, final=False)
    deflate = first + _tiny_dynamic(P[a:s]) + f.bytes()
    assert zlib.decompress(deflate, -15) == text
    return gzip_frame(deflate, text), text, len(first)


def straddling_copy_member(body: bytes):
    """(gzip member, its text, compressed bytes in front of the crafted chunk).  The chunk's first copy starts 20 bytes in
    front of the chunk and runs 40 bytes into it."""
    lines = _lines(body)
    P = b"".join(lines[:60])
    last = lines[59]
    D = b"".join(lines[10:24]) + last[:-20]
    f = FixedBlocks().begin().match(60, len(D) + 20).literals(lines[10][40:]).end().begin(True).end().finish()
    text = P + D + last[-20:] + lines[10]
    first = raw_deflate(P, final=False)
    deflate = first + _tiny_dynamic(D) + f.bytes()
    assert zlib.decompress(deflate, -15) == text
    return gzip_frame(deflate, text), text, len(first)


def too_far_back_member() -> bytes:
    """A member whose first copy reaches in front of its start."""
    f = FixedBlocks().begin(True).literals(b"abc").match(10, 100).end().finish()
    return gzip_frame(f.bytes(), b"")
