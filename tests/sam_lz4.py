"""lz4 copies of a SAM text for the reader, command and device tests: a ctypes binding of the machine's liblz4 (where there
is one) under chosen settings; a pure-Python walker of frames, blocks and sequences, by which tests state what their inputs
contain and where to damage them; and a frame and block writer in plain Python for what the compressor does not emit --
stored blocks, chosen literal and match lengths and offsets, blocks whose bytes end inside a structure, frames with and
without each checksum and a content size, empty and skippable frames, several frames back to back.  The committed
compressor-made inputs lie in tests/golden/lz4 (made by make_inputs.py there).  Test infrastructure only."""
import ctypes as C
import ctypes.util
import hashlib
import os
import random
import struct

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)
from tests.sam_zst import case_text, case_workload, cut_lines  # noqa: F401  (the suite's own texts)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4")
MAGIC = b"\x04\x22\x4d\x18"
LEGACY = b"\x02\x21\x4c\x18"
M32 = (1 << 32) - 1
CHUNK = 2048   # (lz4_decode.hip: kLz4Chunk, the bytes k_lz4_tokens stages at a time)


# ---- liblz4, if the machine has it
class _FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class _Preferences(C.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


def _load():
    for name in ("liblz4.so.1", ctypes.util.find_library("lz4")):
        if not name:
            continue
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        lib.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.POINTER(_Preferences)]
        lib.LZ4F_compressFrameBound.restype = C.c_size_t
        lib.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(_Preferences)]
        lib.LZ4F_compressFrame.restype = C.c_size_t
        lib.LZ4F_isError.argtypes = [C.c_size_t]
        lib.LZ4_decompress_safe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        lib.LZ4_decompress_safe.restype = C.c_int
        return lib
    return None


LIB = _load()


def compress(text: bytes, block_id=0, linked=False, level=0, block_sums=False, content_size=False, checksum=False) -> bytes:
    """One frame of LZ4F_compressFrame's (block_id 0: the library's default, 4..7: 64 KiB .. 4 MiB).  The library lowers the
    block size to fit a small input and writes a one-block frame as independent: ask walk() what came out."""
    p = _Preferences()
    p.frameInfo.blockSizeID, p.frameInfo.blockMode = block_id, 0 if linked else 1
    p.frameInfo.contentChecksumFlag, p.frameInfo.blockChecksumFlag = int(checksum), int(block_sums)
    p.frameInfo.contentSize = len(text) if content_size else 0
    p.compressionLevel = level
    cap = LIB.LZ4F_compressFrameBound(len(text), C.byref(p))
    out = C.create_string_buffer(cap)
    n = LIB.LZ4F_compressFrame(out, cap, text, len(text), C.byref(p))
    assert not LIB.LZ4F_isError(n)
    return out.raw[:n]


def decompress_safe(block: bytes, cap: int):
    """LZ4_decompress_safe on one block's bytes: its text, or None where it refuses them."""
    out = C.create_string_buffer(max(cap, 1))
    n = LIB.LZ4_decompress_safe(block, out, len(block), cap)
    return None if n < 0 else out.raw[:n]


# ---- XXH32 (seed 0)
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data: bytes) -> int:
    n, p = len(data), 0
    if n >= 16:
        v = [(_P1 + _P2) & M32, _P2, 0, (-_P1) & M32]
        while p + 16 <= n:
            for i, w in enumerate(struct.unpack_from("<4I", data, p)):
                v[i] = (_rotl((v[i] + w * _P2) & M32, 13) * _P1) & M32
            p += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M32
    else:
        h = _P5
    h = (h + n) & M32
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, p)[0] * _P3) & M32, 17) * _P4) & M32
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * _P5) & M32, 11) * _P1) & M32
        p += 1
    h ^= h >> 15
    h = h * _P2 & M32
    h ^= h >> 13
    h = h * _P3 & M32
    return h ^ (h >> 16)


# ---- the walker
class Bad(Exception):
    """What the Python walker and decoder refuse, in the host reader's words (lz4_frame.h: status_text)."""


def sequences(block: bytes):
    """A compressed block's sequences: ([(literal length, offset, match length)], the last sequence's literal length)."""
    p, n, out = 0, len(block), []

    def length(v):
        nonlocal p
        if v == 15:
            while True:
                if p >= n:
                    raise Bad("a block that ends inside a length")
                b = block[p]
                p += 1
                v += b
                if b != 255:
                    break
        return v

    while True:
        if p >= n:
            raise Bad("a block that ends behind a match")
        tok = block[p]
        p += 1
        ll = length(tok >> 4)
        if ll > n - p:
            raise Bad("a block that ends inside its literals")
        p += ll
        if p == n:
            return out, ll
        if n - p < 2:
            raise Bad("a block that ends inside an offset")
        off = block[p] | (block[p + 1] << 8)
        p += 2
        if off == 0:
            raise Bad("an offset of 0")
        out.append((ll, off, length(tok & 15) + 4))


def copy_match(out: bytearray, off: int, ml: int):
    if off >= ml:
        out += out[len(out) - off:len(out) - off + ml]
    else:
        out += (bytes(out[-off:]) * (ml // off + 1))[:ml]


def decode_block(block: bytes, out: bytearray, lo: int):
    """The block's text behind `out`, whose bytes from `lo` on a match may reach."""
    seqs, last = sequences(block)
    p = 0
    for ll, off, ml in seqs:
        p += 1 + (0 if ll < 15 else (ll - 15) // 255 + 1)
        out += block[p:p + ll]
        p += ll + 2 + (0 if ml < 19 else (ml - 19) // 255 + 1)
        if off > len(out) - lo:
            raise Bad("an offset beyond the frame's start")
        copy_match(out, off, ml)
    out += block[len(block) - last:]


def walk(blob: bytes):
    """The frames of `blob`: [{"at", "skippable", "linked", "block_sums", "content_size", "block_max", "end_at" (the end mark),
    "checksum_at", "blocks": [{"at" (of the header), "stored", "size", "sum_at"}]}]."""
    frames, p = [], 0
    while p < len(blob):
        magic = struct.unpack_from("<I", blob, p)[0]
        if (magic & 0xfffffff0) == 0x184D2A50:
            n = struct.unpack_from("<I", blob, p + 4)[0]
            frames.append({"at": p, "skippable": True, "blocks": []})
            p += 8 + n
            continue
        assert blob[p:p + 4] == MAGIC, p
        flg, bd = blob[p + 4], blob[p + 5]
        f = {"at": p, "skippable": False, "blocks": [], "linked": not flg & 0x20, "block_sums": bool(flg & 0x10), "content_size": None,
             "block_max": 1 << (8 + 2 * (bd >> 4)), "checksum_at": None}
        q = p + 6
        if flg & 8:
            f["content_size"] = struct.unpack_from("<Q", blob, q)[0]
            q += 8
        f["hc_at"] = q
        q += 1
        while True:
            h = struct.unpack_from("<I", blob, q)[0]
            if h == 0:
                f["end_at"] = q
                q += 4
                break
            b = {"at": q, "stored": bool(h >> 31), "size": h & 0x7fffffff, "sum_at": None}
            q += 4 + b["size"]
            if f["block_sums"]:
                b["sum_at"] = q
                q += 4
            f["blocks"].append(b)
        if flg & 4:
            f["checksum_at"] = q
            q += 4
        frames.append(f)
        p = q
    return frames


def decode(blob: bytes) -> bytes:
    """The text of `blob` by the Python walker and decoder (no check is verified: the tests' statement of what an input holds)."""
    text = bytearray()
    for f in walk(blob):
        start = len(text)
        for b in f["blocks"]:
            body = blob[b["at"] + 4:b["at"] + 4 + b["size"]]
            if b["stored"]:
                text += body
            else:
                decode_block(body, text, start if f["linked"] else len(text))
    return bytes(text)


def census(blob: bytes) -> dict:
    """What `blob` holds, by the walker."""
    out = {"frames": 0, "skippable": 0, "linked": 0, "stored": 0, "compressed": 0, "sequences": 0, "block_sums": 0, "content_sums": 0,
           "max_offset": 0}
    for f in walk(blob):
        out["skippable" if f["skippable"] else "frames"] += 1
        if f["skippable"]:
            continue
        out["linked"] += int(f["linked"])
        out["content_sums"] += int(f["checksum_at"] is not None)
        for b in f["blocks"]:
            out["stored" if b["stored"] else "compressed"] += 1
            out["block_sums"] += int(b["sum_at"] is not None)
            if not b["stored"]:
                seqs, _ = sequences(blob[b["at"] + 4:b["at"] + 4 + b["size"]])
                out["sequences"] += len(seqs)
                out["max_offset"] = max([out["max_offset"]] + [s[1] for s in seqs])
    return out


# ---- the writer
def frame_header(linked=False, block_sums=False, content_size=None, checksum=False, block_id=4, version=1, reserved=0, dict_id=None,
                 bd_reserved=0, wrong_hc=False) -> bytes:
    flg = (version << 6) | (0 if linked else 0x20) | (0x10 if block_sums else 0) | (8 if content_size is not None else 0) | (4 if checksum else 0)
    flg |= (2 if reserved else 0) | (0 if dict_id is None else 1)
    d = bytes([flg, (block_id << 4) | bd_reserved])
    if content_size is not None:
        d += struct.pack("<Q", content_size)
    if dict_id is not None:
        d += struct.pack("<I", dict_id)
    return MAGIC + d + bytes([((xxh32(d) >> 8) & 0xff) ^ (1 if wrong_hc else 0)])


def _ext(v: int) -> bytes:
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq_block(seqs, tail: bytes = b"", final=True) -> bytes:
    """A compressed block's bytes: seqs = [(literals, offset, match length)], then the last sequence's literals (final=False:
    no last sequence -- the bytes end right behind the last match)."""
    out = bytearray()
    for lits, off, ml in seqs:
        ll, m = len(lits), ml - 4
        out.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= 15:
            out += _ext(ll - 15)
        out += lits
        out += struct.pack("<H", off)
        if m >= 15:
            out += _ext(m - 15)
    if final:
        out.append(min(len(tail), 15) << 4)
        if len(tail) >= 15:
            out += _ext(len(tail) - 15)
        out += tail
    return bytes(out)


def sequences_of(history: bytes, data: bytes):
    """A greedy parse of `data` behind `history` (hash of 4 bytes, the last position only): (seqs, tail) for seq_block."""
    buf = history + data
    base = len(history)
    table, seqs, anchor, i, n = {}, [], base, base, len(buf)
    for j in range(max(0, base - 65535), base - 3):
        table[buf[j:j + 4]] = j
    while i + 4 <= n - 5:   # (the last 5 bytes stay literals, as the format's own compressors leave them)
        key = buf[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is None or i - j > 65535:
            i += 1
            continue
        ml = 4
        while i + ml < n - 5 and buf[j + ml] == buf[i + ml]:
            ml += 1
        seqs.append((buf[anchor:i], i - j, ml))
        i += ml
        anchor = i
    return seqs, buf[anchor:]


class Frame:
    """One frame being written: its blocks' bytes and the text they decode to (Python's own decoding of them)."""

    def __init__(self, linked=False, block_id=4):
        self.linked, self.block_id, self.blocks, self.out = linked, block_id, [], bytearray()

    def stored(self, data: bytes, step=50_000):
        for i in range(0, len(data), step):
            self.blocks.append((True, data[i:i + step]))
        self.out += data
        return self

    def compressed(self, seqs, tail=b"", final=True):
        body = seq_block(seqs, tail, final)
        self.blocks.append((False, body))
        decode_block(body, self.out, 0 if self.linked else len(self.out))
        return self

    def packed(self, data: bytes, step=60_000):
        """`data` as compressed blocks of a greedy parse."""
        for i in range(0, len(data), step):
            hist = bytes(self.out[-65535:]) if self.linked else b""
            seqs, tail = sequences_of(hist, data[i:i + step])
            self.compressed(seqs, tail)
        return self

    def bytes(self, block_sums=False, content_size=False, checksum=True, wrong_sum=False, wrong_size=False, wrong_block_sum=False) -> bytes:
        size = len(self.out) + (1 if wrong_size else 0) if content_size or wrong_size else None
        parts = [frame_header(self.linked, block_sums, size, checksum, self.block_id)]
        for k, (stored, body) in enumerate(self.blocks):
            parts.append(struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + body)
            if block_sums:
                parts.append(struct.pack("<I", xxh32(body) ^ (1 if wrong_block_sum and k == len(self.blocks) // 2 else 0)))
        parts.append(struct.pack("<I", 0))
        if checksum:
            parts.append(struct.pack("<I", xxh32(bytes(self.out)) ^ (1 if wrong_sum else 0)))
        return b"".join(parts)


def skippable(payload: bytes = b"between two frames", nibble=7) -> bytes:
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


def written_copies(text: bytes) -> dict:
    """The Python-written forms of `text`: {kind: blob}."""
    a, b, c = cut_lines(text, 3)
    return {
        "stored_blocks": Frame().stored(text).bytes(checksum=False),
        "packed_independent": Frame().packed(text).bytes(block_sums=True, content_size=True),
        "packed_linked": Frame(linked=True).packed(text).bytes(content_size=True, checksum=False),
        "linked_mixed": Frame(linked=True).stored(a).packed(b).stored(c[:100]).packed(c[100:]).bytes(block_sums=True),
        "frames": (Frame().packed(a).bytes(content_size=True) + Frame().bytes() + skippable() + Frame(linked=True).packed(b).bytes(checksum=False)
                   + skippable(b"", 0) + Frame().stored(c, step=7_000).bytes(block_sums=True, checksum=False) + Frame().bytes(content_size=True, checksum=False)),
    }


# ---- the directed inputs ----------------------------------------------------------------------------------------------------
_FILL = bytes(random.Random(5).choice(b"ACGTNacgtn !#0123456789:;<=>?IJKLMNOPQRST~") for _ in range(1 << 16))


def letters(n: int, at: int = 0) -> bytes:
    at %= 4099
    return (_FILL[at:] + _FILL * (n // len(_FILL) + 1))[:n]


LIT_LENGTHS = (0, 14, 15, 270, 524, 525)
MATCH_LENGTHS = (4, 18, 19, 273, 274, 529)
SEQ_COUNTS = (0, 1, 63, 64, 65, 128)


def staging_frame(k_most=4096):
    """Blocks 0 .. k_most of a linked frame: block k = k literal bytes, a short match, then the same sequence with 3-byte
    extensions of both lengths (525 literals, a match of 529) -- so every structure of it lies across every boundary of the
    kernel's staging (CHUNK = 2048 bytes at a time, at any alignment of the block's first byte)."""
    f = Frame(linked=True).stored(b"@CO\tstaging\n@CO\t")
    for k in range(k_most + 1):
        f.compressed([(letters(k, k), 4, 4), (letters(516, k) + b"\n@CO\t" + letters(4, k), 3, 529)])
    return f.stored(b"\n")


def INPUTS(header: bytes, records: bytes, staging=True) -> dict:
    """{name: (lz4 bytes, text, skip)}: good inputs, each a directed structure in comment lines between the SAM header and the
    records; every frame states a content checksum, which is what turns one wrong byte of the text into a failure."""
    out = {}

    def add(name, *frames, **kw):
        text = b"".join(bytes(f.out) if isinstance(f, Frame) else b"" for f in frames)
        blob = b"".join(f.bytes(**kw) if isinstance(f, Frame) else f for f in frames)
        out[name] = (blob, text, text.index(records))

    add("stored_only", Frame().stored(header + records, step=9_000))
    # a linked frame that mixes stored and compressed blocks, with a match into a stored block
    f = Frame(linked=True).stored(header).stored(b"@CO\t" + letters(300) + b"\n")
    f.compressed([(b"@CO\t", 200, 150)], b"\n").stored(b"@CO\tstored again\n").compressed([(b"", 17, 17)], b"").packed(records)
    add("linked_mixed", f, block_sums=True)
    # a match that reaches 65 535 bytes back through three short blocks
    f = Frame(linked=True).stored(header).stored(b"@CO\t" + letters(65_600) + b"\n", step=65_536)
    f.stored(b"@CO\tone\n").stored(b"@CO\ttwo\n").stored(b"@CO\tthree\n").compressed([(b"@CO\t", 65_535, 40)], b"\n").packed(records)
    add("reach_65535", f)
    # a match to the frame's first byte, behind another frame: what lies in front of the frame is not the match's to reach
    f = Frame(linked=True).stored(b"@CO\tfirst\n").compressed([(b"", 10, 10)], b"").packed(records)
    add("first_byte", Frame().stored(header), f)
    # literal and match lengths around the nibble's and the extension bytes' edges, in one comment line
    seqs = [(b"@CO\t" + letters(266), 5, 4)]
    seqs += [(letters(ll, 7 * ll), 1 + ml % 7, ml) for ll, ml in zip(LIT_LENGTHS, MATCH_LENGTHS)]
    seqs += [(letters(ll, 3 * ll), 2, ml) for ll, ml in zip(LIT_LENGTHS, reversed(MATCH_LENGTHS))]
    add("lengths", Frame().stored(header).compressed(seqs, b"\n").packed(records))
    add("offsets_1_2_3", Frame().stored(header).compressed([(b"@CO\tA", 1, 1_000), (b"CG", 2, 777), (b"TNA", 3, 4_000)], b"\n").packed(records))
    # blocks of 0, 1, 63, 64, 65 and 128 sequences: the edges of the 64-at-a-time store
    f = Frame().stored(header)
    for n in SEQ_COUNTS:
        f.compressed([(b"@CO\t" + letters(9, n), 3, 5)] * min(n, 1) + [(letters(2, k), 1 + k % 9, 4 + k % 3) for k in range(n - 1)], b"\n" if n else b"@CO\tnone\n")
    add("sequence_counts", f.packed(records))
    # a block that ends in a token of zero literals
    add("zero_literals_last", Frame().stored(header).compressed([(b"@CO\tab\n", 7, 7)], b"").packed(records))
    if staging:
        f = staging_frame()
        add("staging", Frame().stored(header), f, Frame(linked=True).packed(records))
    # frames with and without each checksum and a content size; an empty frame; frames back to back with skippable frames
    for k in range(8):
        kw = dict(block_sums=bool(k & 1), content_size=bool(k & 2), checksum=bool(k & 4))
        add("flags_%d" % k, Frame(linked=bool(k & 1)).stored(header).packed(records), **kw)
    add("empty_first", Frame(), Frame().stored(header + records))
    a, b = records[:len(records) // 2], records[len(records) // 2:]
    add("frames", Frame().stored(header), skippable(), Frame(linked=True).packed(a), Frame(), skippable(b"", 1), Frame().packed(b), skippable(b"end"))
    return out


def INVALID(header: bytes, records: bytes) -> dict:
    """{name: (lz4 bytes, the cause in the host reader's words)}: directed errors, each the only fault of its input."""
    out = {}
    head = lambda linked=False: Frame(linked).stored(header)   # noqa: E731

    def broken(f, body, words, front=b""):
        """`body` as the compressed block behind f's (the Python decoder is not asked: it refuses it too), and the records."""
        f.blocks.append((False, body))
        f.blocks.append((True, records))
        return front + f.bytes(checksum=False), words

    # one byte beyond the frame's first byte: a byte of the frame in front, which is there in the round's text
    out["beyond_first_byte"] = broken(Frame(linked=True).stored(b"@CO\tfirst\n"), seq_block([(b"", 11, 10)], b"\n"), "an offset beyond the frame's start",
                                      front=Frame().stored(header).bytes())
    out["offset_zero"] = broken(head(), seq_block([(b"@CO\tabcdef", 0, 6)], b"\n"), "an offset of 0")
    f = head().stored(b"@CO\t" + letters(100) + b"\n")
    out["independent_reaches_front"] = broken(f, seq_block([(b"@CO\t", 50, 20)], b"\n"), "an offset beyond the frame's start, or beyond the block's")
    good = seq_block([(b"@CO\t" + letters(300), 7, 300)], letters(20) + b"\n")
    ends = {"inside_extension": (good[:2], "a block that ends inside a length"),
            "inside_literals": (good[:100], "a block that ends inside its literals"),
            "after_one_offset_byte": (good[:3 + 304 + 1], "a block that ends inside an offset"),
            "inside_match_extension": (good[:3 + 304 + 2], "a block that ends inside a length"),
            "behind_match": (seq_block([(b"@CO\t" + letters(300), 7, 300)], final=False), "a block that ends behind a match")}
    for name, (body, words) in ends.items():
        out["ends_" + name] = broken(head(), body, words)
    return out


def UNSAFE_BUT_TAKEN() -> dict:
    """{name: (block, text)}: blocks that LZ4_decompress_safe refuses (its end-of-block rules: the last match starts 12 bytes
    or more in front of the end, the last 5 bytes are literals) and both decoders here take -- they agree with each other."""
    out = {}
    for k in (3, 4, 5, 6, 7):   # literals ending k bytes before the block's end with a short match behind them: its offset, the last token, k - 3 literals
        body = seq_block([(b"@CO\t" + letters(30), 4, 4)], letters(k - 3))
        text = bytearray()
        decode_block(body, text, 0)
        out["short_end_%d" % k] = (body, bytes(text))
    return out


def digest(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()[:16]
