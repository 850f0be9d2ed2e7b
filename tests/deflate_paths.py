"""An inflater of gzip members in plain Python that counts the paths an input takes, written from RFC 1951 / RFC 1952 (the
walker blocks() of tests/sam_deflate.py grown into a decoder): decode(blob, chunk_bits=()) -> (text, Counter of named paths),
all_paths() the names there are, Bad what it raises on a stream it refuses (zlib's rules: slimm_amd/csrc/deflate_stream.h).
chunk_bits: the bit offsets in the blob at which the device decoder starts a chunk (gzip_decode.hip) -- a copy is counted by
where its source lies as seen from its chunk's start, and so are the text bytes whose source lies in front of their chunk,
which the device writes as markers and resolves later.  chunk_starts() gives those offsets for a SLIMM_FORCE gzip_chunk=N.
tests/deflate_directed.py writes inputs for chosen paths.  Test infrastructure only."""
import struct
import zlib
from collections import Counter

import numpy as np

from tests.sam_deflate import _DBASE, _DEXT, _LBASE, _LEXT, _ORDER

WINDOW = 32768


class Bad(Exception):
    pass


def all_paths():
    p = ["stored:len:0", "stored:len:65535"] + [f"stored:pad:{k}" for k in range(8)]
    p += [f"{t}:{f}" for t in ("fixed", "dynamic") for f in ("final", "not_final", "empty")]
    p += ["hlit:257", "hlit:286", "hdist:1", "hdist:30", "hclen:4", "hclen:19"]
    p += [f"cl:{k}" for k in range(16)] + ["cl:16:rep3", "cl:16:rep6", "cl:17:rep3", "cl:17:rep10", "cl:18:rep11", "cl:18:rep138", "cl:repeat_across_hlit"]
    p += [f"lit_len:{k}" for k in range(1, 16)] + [f"dist_len:{k}" for k in range(1, 16)]
    p += ["set:lit:complete", "set:lit:one_code", "set:dist:one_code", "set:dist:none", "lit:below_144", "lit:from_144"]
    p += [f"len_sym:{s}:{e}" for s in range(257, 286) for e in ("zeros", "ones")] + ["len258:as_285", "len258:as_284+31"]
    p += [f"dist_sym:{s}:{e}" for s in range(30) for e in ("zeros", "ones")]
    p += [f"copy:inside:dist{k}" for k in range(1, 9)] + ["copy:inside:dist>8", "copy:wholly_in_front", "copy:across_start:dist<8",
                                                          "copy:across_start:dist>=8", "copy:dist32768_from_n0", "copy:of_unresolved"]
    p += [f"copy:tail:{k}" for k in range(1, 8)] + ["copy:from_stored_block", "copy:from_earlier_block_of_chunk", "bytes:from_in_front_of_chunk"]
    return p


class _Reader:
    """Bits in the stream's order (the lowest bit of a byte first): a Huffman code reads as its bits from the highest on."""

    def __init__(self, blob, bit=0):
        self.bits = (np.unpackbits(np.frombuffer(blob, dtype=np.uint8), bitorder="little") + 48).astype(np.uint8).tobytes().decode("ascii")
        self.pos = bit

    def get(self, k):
        if self.pos + k > len(self.bits):
            raise Bad("truncated")
        v = int(self.bits[self.pos:self.pos + k][::-1], 2) if k else 0
        self.pos += k
        return v

    def symbol(self, codes, what):
        for ln in range(1, 16):
            s = codes.get(self.bits[self.pos:self.pos + ln])
            if s is not None:
                if self.pos + ln > len(self.bits):
                    break
                self.pos += ln
                return s
        raise Bad("truncated" if self.pos + 15 > len(self.bits) else f"invalid {what} code")


def _codes(lengths):
    """({code as a bit string: symbol}, what is left of the code space in units of 2^-15, the longest code)."""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[format(nxt[ln], "0%db" % ln)] = s
            nxt[ln] += 1
    left = (1 << 15) - sum(count[ln] << (15 - ln) for ln in range(1, 16))
    return out, left, max(lengths) if lengths else 0


_FIXED = (_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)[0], _codes([5] * 30)[0])


def _dynamic(r, c):
    hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    if hlit > 286 or hdist > 30:
        raise Bad("too many length or distance symbols")
    cl = [0] * 19
    for i in range(hclen):
        cl[_ORDER[i]] = r.get(3)
    codes, left, _ = _codes(cl)
    if left != 0:
        raise Bad("invalid code lengths set")
    lens, paths = [], [f"hlit:{hlit}", f"hdist:{hdist}", f"hclen:{hclen}"]
    while len(lens) < hlit + hdist:
        s = r.symbol(codes, "code lengths")
        if s < 16:
            lens.append(s)
            paths.append(f"cl:{s}")
            continue
        if s == 16 and not lens:
            raise Bad("invalid bit length repeat")
        rep = 3 + r.get(2) if s == 16 else 3 + r.get(3) if s == 17 else 11 + r.get(7)
        if len(lens) + rep > hlit + hdist:
            raise Bad("invalid bit length repeat")
        paths.append(f"cl:{s}:rep{rep}")
        if len(lens) < hlit < len(lens) + rep:
            paths.append("cl:repeat_across_hlit")
        lens += [lens[-1] if s == 16 else 0] * rep
    if lens[256] == 0:
        raise Bad("invalid code -- missing end-of-block")
    lit, left, mx = _codes(lens[:hlit])
    if left < 0 or (left > 0 and mx != 1):
        raise Bad("invalid literal/lengths set")
    paths.append("set:lit:complete" if left == 0 else "set:lit:one_code")
    dist, left, mx = _codes(lens[hlit:])
    if left < 0 or (left > 0 and mx > 1):
        raise Bad("invalid distances set")
    if mx == 0:
        paths.append("set:dist:none")
    elif left > 0:
        paths.append("set:dist:one_code")
    paths += [f"lit_len:{ln}" for ln in set(lens[:hlit]) if ln] + [f"dist_len:{ln}" for ln in set(lens[hlit:]) if ln]
    for p in paths:
        c[p] += 1
    return lit, dist, "set:lit:complete" in paths


class _Chunk:
    """What the device's Out16 knows of a chunk: its bytes so far, and which of them are markers."""

    def __init__(self, avail):
        self.n, self.avail, self.unresolved, self.kind, self.block_at = 0, avail, bytearray(), bytearray(), 0


def _copy(c, ch, length, dist, total):
    """A copy counted by where its source lies as seen from the chunk's start (Out16::copy's branches)."""
    n = ch.n
    if dist > total:
        raise Bad("invalid distance too far back")
    front = min(length, max(0, dist - n))     # bytes written as markers: their source lies in front of the chunk
    if front:
        c["copy:wholly_in_front" if front == length else "copy:across_start:dist<8" if dist < 8 else "copy:across_start:dist>=8"] += 1
        c["copy:dist32768_from_n0"] += n == 0 and dist == WINDOW
    else:
        c[f"copy:inside:dist{dist}" if dist <= 8 else "copy:inside:dist>8"] += 1
    rest = length - front
    if rest and dist >= 8 and rest % 8:
        c[f"copy:tail:{rest % 8}"] += 1
    marks = stored = 0
    for k in range(length):
        src = n + k - dist
        u = 1 if src < 0 else ch.unresolved[src]
        if src >= 0:
            marks += ch.unresolved[src]
            stored += ch.kind[src] == 0
        ch.unresolved.append(u)
        ch.kind.append(3)
    c["copy:of_unresolved"] += marks > 0
    c["copy:from_stored_block"] += stored > 0
    c["copy:from_earlier_block_of_chunk"] += 0 <= n - dist < ch.block_at
    ch.n += length


def inflate(r, c, text, chunk_bits=(), member_at=0, blocks=None):
    """The blocks of one deflate stream from r.pos on, their text appended to `text` (the member's starts at member_at);
    blocks, when given, gets (bit offset, type, final, text bytes, a non-final dynamic block with a complete literal code)."""
    ch = _Chunk(0)
    while True:
        at = r.pos
        if at in chunk_bits:
            c["bytes:from_in_front_of_chunk"] += sum(ch.unresolved)
            ch = _Chunk(min(WINDOW, len(text) - member_at))
            c["count:chunks"] += 1
        ch.block_at, before, complete = ch.n, len(text), False
        final, typ = r.get(1), r.get(2)
        if typ == 3:
            raise Bad("invalid block type")
        if typ == 0:
            pad = -r.pos % 8
            r.pos += pad
            n, nn = r.get(16), r.get(16)
            if n ^ 0xffff != nn:
                raise Bad("invalid stored block lengths")
            if r.pos + 8 * n > len(r.bits):
                raise Bad("truncated")
            c[f"stored:pad:{pad}"] += 1
            c[f"stored:len:{n}"] += 1
            c["count:stored"] += 1
            for _ in range(n):
                text.append(r.get(8))
            ch.unresolved += bytes(n)
            ch.kind += bytes(n)
            ch.n += n
        else:
            name = "fixed" if typ == 1 else "dynamic"
            if typ == 1:
                lit, dist = _FIXED
            else:
                lit, dist, complete = _dynamic(r, c)
            while True:
                s = r.symbol(lit, "literal/length")
                if s < 256:
                    c["lit:below_144" if s < 144 else "lit:from_144"] += 1
                    text.append(s)
                    ch.unresolved.append(0)
                    ch.kind.append(typ)
                    ch.n += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise Bad("invalid literal/length code")
                e = r.get(_LEXT[s - 257])
                length = _LBASE[s - 257] + e
                c[f"len_sym:{s}:zeros"] += e == 0
                c[f"len_sym:{s}:ones"] += e == (1 << _LEXT[s - 257]) - 1
                if length == 258:
                    c["len258:as_285" if s == 285 else "len258:as_284+31"] += 1
                d = r.symbol(dist, "distance")
                if d > 29:
                    raise Bad("invalid distance code")
                e = r.get(_DEXT[d])
                c[f"dist_sym:{d}:zeros"] += e == 0
                c[f"dist_sym:{d}:ones"] += e == (1 << _DEXT[d]) - 1
                _copy(c, ch, length, _DBASE[d] + e, len(text) - member_at)
                for _ in range(length):
                    text.append(text[-(_DBASE[d] + e)])
            c[f"{name}:{'final' if final else 'not_final'}"] += 1
            c[f"{name}:empty"] += len(text) == before
            c[f"count:{name}"] += 1
        if blocks is not None:
            blocks.append((at, typ, bool(final), len(text) - before, complete and not final))
        if final:
            c["bytes:from_in_front_of_chunk"] += sum(ch.unresolved)
            return


def _member_header(blob, at):
    if len(blob) - at < 10:
        raise Bad("truncated")
    if blob[at:at + 3] != b"\x1f\x8b\x08" or blob[at + 3] & 0xe0:
        raise Bad("no gzip member")
    flg, p = blob[at + 3], at + 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", blob, p)[0]
    for f in (8, 16):
        if flg & f:
            p = blob.index(b"\0", p) + 1
    return p + (2 if flg & 2 else 0)


def decode(blob: bytes, chunk_bits=()):
    c, out, at = Counter(), bytearray(), 0
    r = _Reader(blob)
    chunk_bits = set(chunk_bits)
    while at < len(blob):
        start = len(out)
        r.pos = _member_header(blob, at) * 8
        c["count:chunks"] += 1
        inflate(r, c, out, chunk_bits - {r.pos}, start)
        at = (r.pos + 7) // 8
        if at + 8 > len(blob):
            raise Bad("truncated")
        crc, isize = struct.unpack_from("<II", blob, at)
        if crc != zlib.crc32(bytes(out[start:])):
            raise Bad("incorrect data check")
        if isize != (len(out) - start) & 0xffffffff:
            raise Bad("incorrect length check")
        at += 8
        c["count:members"] += 1
    return bytes(out), +c


def candidates(blob: bytes):
    """(the first block's bit offset, those of the non-final dynamic blocks whose literal/length code is complete) of a
    one-member file: what the device's search for chunk starts finds (and, by chance, other offsets: its `dropped` says when)."""
    r, blocks = _Reader(blob), []
    r.pos = first = _member_header(blob, 0) * 8
    inflate(r, Counter(), bytearray(), blocks=blocks)
    return first, [b[0] for b in blocks if b[4]]


def chunk_starts(blob: bytes, chunk_bytes: int):
    """The chunk starts the device takes in a one-round run of a one-member file under SLIMM_FORCE gzip_chunk=chunk_bytes:
    the member's first block, and the first candidate at or behind every chunk_bytes compressed bytes."""
    first, cand = candidates(blob)
    starts, cb, target = [first], chunk_bytes * 8, first + chunk_bytes * 8
    while True:
        later = [b for b in cand if b >= target]
        if not later:
            return starts
        starts.append(later[0])
        target = first + ((later[0] - first) // cb + 1) * cb
