"""zstd copies of a SAM text for the reader, command and device tests: a ctypes binding of the machine's libzstd (where
there is one) under chosen settings; a pure-Python walker of frames and blocks, by which tests state what their inputs
contain and where to damage them; and a frame writer in plain Python for what the compressor does not emit on SAM text --
raw blocks only, RLE blocks, frames with and without content size, checksum and window descriptor, empty and skippable
frames, several frames back to back, one hand-made compressed block.  The committed compressor-made inputs lie in
tests/golden/zstd (made by make_inputs.py there).  Test infrastructure only."""
import ctypes as C
import ctypes.util
import os
import struct

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd")
MAGIC = b"\x28\xb5\x2f\xfd"
M64 = (1 << 64) - 1


# ---- libzstd, if the machine has it
def _load():
    for name in ("libzstd.so.1", ctypes.util.find_library("zstd")):
        if not name:
            continue
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        lib.ZSTD_createCCtx.restype = C.c_void_p
        lib.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        lib.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.ZSTD_CCtx_setParameter.restype = C.c_size_t
        lib.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.ZSTD_compress2.restype = C.c_size_t
        lib.ZSTD_compressBound.argtypes = [C.c_size_t]
        lib.ZSTD_compressBound.restype = C.c_size_t
        lib.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.ZSTD_decompress.restype = C.c_size_t
        lib.ZSTD_isError.argtypes = [C.c_size_t]
        return lib
    return None


LIB = _load()


def compress(text: bytes, level=3, window_log=0, content_size=True, checksum=True) -> bytes:
    """One frame of libzstd's (parameter 100 = level, 101 = windowLog, 200 = content size flag, 201 = checksum flag)."""
    cctx = LIB.ZSTD_createCCtx()
    try:
        for k, v in ((100, level), (101, window_log), (200, int(content_size)), (201, int(checksum))):
            assert not LIB.ZSTD_isError(LIB.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = LIB.ZSTD_compressBound(len(text))
        out = C.create_string_buffer(cap)
        n = LIB.ZSTD_compress2(cctx, out, cap, text, len(text))
        assert not LIB.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        LIB.ZSTD_freeCCtx(cctx)


def decompress(blob: bytes, cap: int) -> bytes:
    """ZSTD_decompress: every frame of `blob`, at most `cap` bytes."""
    out = C.create_string_buffer(max(cap, 1))
    n = LIB.ZSTD_decompress(out, cap, blob, len(blob))
    assert not LIB.ZSTD_isError(n), "ZSTD_decompress failed"
    return out.raw[:n]


# ---- XXH64 (seed 0)
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, v):
    return (_rotl((acc + v * _P2) & M64, 31) * _P1) & M64


def xxh64(data: bytes) -> int:
    n, p = len(data), 0
    if n >= 32:
        v = [(_P1 + _P2) & M64, _P2, 0, (-_P1) & M64]
        while p + 32 <= n:
            for i, w in enumerate(struct.unpack_from("<4Q", data, p)):
                v[i] = _round(v[i], w)
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for x in v:
            h = ((h ^ _round(0, x)) * _P1 + _P4) & M64
    else:
        h = _P5
    h = (h + n) & M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27) * _P1 + _P4) & M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, p)[0] * _P1 & M64), 23) * _P2 + _P3) & M64
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & M64), 11) * _P1) & M64
        p += 1
    h ^= h >> 33
    h = h * _P2 & M64
    h ^= h >> 29
    h = h * _P3 & M64
    return h ^ (h >> 32)


# ---- the walker
def _fse_desc_len(b: bytes, at: int, max_log: int) -> int:
    """Bytes of the FSE table description at b[at:]."""
    bit = at * 8

    def get(k):
        nonlocal bit
        v = (int.from_bytes(b[bit >> 3:(bit >> 3) + 8], "little") >> (bit & 7)) & ((1 << k) - 1)
        bit += k
        return v

    log = get(4) + 5
    assert log <= max_log
    remaining = 1 << log
    while remaining > 0:
        bits = (remaining + 1).bit_length()
        val = get(bits)
        lower = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if (val & lower) < threshold:
            bit -= 1
            val &= lower
        elif val > lower:
            val -= threshold
        proba = val - 1
        remaining -= 1 if proba < 0 else proba
        if proba == 0:
            while get(2) == 3:
                pass
    return (bit + 7) // 8 - at


def walk(blob: bytes):
    """The frames of `blob`: [{"at", "skippable", "window", "content_size", "checksum_at", "blocks": [{"at" (of the header),
    "type" 0 raw / 1 RLE / 2 compressed, "size", "last", and of a compressed block "lit_type" 0..3, "huf_at" (a tree's
    description), "modes" (literal lengths, offsets, match lengths; None without sequences), "n_seq", "fse_at" (the first
    FSE description), "bits_at" (the sequences' bitstream)}]}]."""
    frames, p = [], 0
    while p < len(blob):
        magic = struct.unpack_from("<I", blob, p)[0]
        if (magic & 0xfffffff0) == 0x184D2A50:
            n = struct.unpack_from("<I", blob, p + 4)[0]
            frames.append({"at": p, "skippable": True, "blocks": []})
            p += 8 + n
            continue
        assert blob[p:p + 4] == MAGIC, p
        f = {"at": p, "skippable": False, "blocks": [], "window": None, "content_size": None, "checksum_at": None}
        d = blob[p + 4]
        q = p + 5
        single = (d >> 5) & 1
        if not single:
            w = blob[q]
            q += 1
            f["window"] = (1 << (10 + (w >> 3))) + ((1 << (10 + (w >> 3))) >> 3) * (w & 7)
        q += (0, 1, 2, 4)[d & 3]
        nf = (single, 2, 4, 8)[d >> 6]
        if nf:
            f["content_size"] = int.from_bytes(blob[q:q + nf], "little") + (256 if nf == 2 else 0)
            q += nf
        while True:
            h = int.from_bytes(blob[q:q + 3], "little")
            b = {"at": q, "type": (h >> 1) & 3, "size": h >> 3, "last": bool(h & 1)}
            body = q + 3
            if b["type"] == 2:
                t = blob[body] & 3
                fmt = (blob[body] >> 2) & 3
                b["lit_type"] = t
                if t < 2:
                    hb = (1, 2, 1, 3)[fmt]
                    regen = int.from_bytes(blob[body:body + hb], "little") >> (3 if hb == 1 else 4)
                    comp = regen if t == 0 else 1
                else:
                    hb = (3, 3, 4, 5)[fmt]
                    nb = (10, 10, 14, 18)[fmt]
                    v = int.from_bytes(blob[body:body + hb], "little") >> 4
                    comp = (v >> nb) & ((1 << nb) - 1)
                    b["huf_at"] = body + hb if t == 2 else None
                s = body + hb + comp
                n0 = blob[s]
                if n0 == 0:
                    b["n_seq"], b["modes"] = 0, None
                else:
                    if n0 < 128:
                        b["n_seq"], s = n0, s + 1
                    elif n0 < 255:
                        b["n_seq"], s = ((n0 - 128) << 8) + blob[s + 1], s + 2
                    else:
                        b["n_seq"], s = blob[s + 1] + (blob[s + 2] << 8) + 0x7F00, s + 3
                    m = blob[s]
                    s += 1
                    b["modes"] = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
                    b["mode_byte"] = m
                    b["fse_at"] = None
                    for k, mode in enumerate(b["modes"]):
                        if mode == 1:
                            s += 1
                        elif mode == 2:
                            if b["fse_at"] is None:
                                b["fse_at"] = s
                            s += _fse_desc_len(blob, s, (9, 8, 9)[k])
                    b["bits_at"] = s
            f["blocks"].append(b)
            q = body + (1 if b["type"] == 1 else b["size"])
            if b["last"]:
                break
        if d & 4:
            f["checksum_at"] = q
            q += 4
        frames.append(f)
        p = q
    return frames


def census(blob: bytes) -> dict:
    """What `blob` holds, by the walker: frames, skippable, blocks by type, literals sections by type, tables by mode."""
    out = {"frames": 0, "skippable": 0, "raw": 0, "rle": 0, "compressed": 0, "lit_raw": 0, "lit_rle": 0, "lit_huffman": 0, "lit_treeless": 0,
           "predefined": 0, "rle_tables": 0, "fse_tables": 0, "repeated": 0, "mode_bytes": set()}
    for f in walk(blob):
        out["skippable" if f["skippable"] else "frames"] += 1
        for b in f["blocks"]:
            out[("raw", "rle", "compressed")[b["type"]]] += 1
            if b["type"] == 2:
                out[("lit_raw", "lit_rle", "lit_huffman", "lit_treeless")[b["lit_type"]]] += 1
                if b["modes"]:
                    out["mode_bytes"].add(b["mode_byte"])
                    for m in b["modes"]:
                        out[("predefined", "rle_tables", "fse_tables", "repeated")[m]] += 1
    return out


# ---- the writer
def frame_header(content_size=None, checksum=False, window_log=None, dict_id=None) -> bytes:
    """Magic and header.  window_log None: a single segment (the content size is then stated, in 8 bytes); else a window
    descriptor of 1 << window_log, and the content size in 8 bytes when given."""
    d = (4 if checksum else 0) | (0 if dict_id is None else 1)
    if window_log is None:
        assert content_size is not None
        d |= 0x20 | 0xC0
        body = b""
    else:
        d |= 0xC0 if content_size is not None else 0
        body = bytes([(window_log - 10) << 3])
    if dict_id is not None:
        body += bytes([dict_id])
    if content_size is not None:
        body += struct.pack("<Q", content_size)
    return MAGIC + bytes([d]) + body


def block(kind: int, payload: bytes, size=None, last=False) -> bytes:
    n = len(payload) if size is None else size
    return struct.pack("<I", (n << 3) | (kind << 1) | int(last))[:3] + payload


def blocks_of(text: bytes, step=50_000, rle=True):
    """Raw blocks of at most `step` bytes; where the text has a run of one byte of 8 or more, an RLE block for it."""
    out, p, n = [], 0, len(text)
    while p < n:
        run = 1
        while rle and p + run < n and text[p + run] == text[p] and run < step:
            run += 1
        if run >= 8:
            out.append((1, text[p:p + 1], run))
            p += run
            continue
        q = p + 1
        while q < n and q - p < step:
            if rle and q + 8 <= n and text[q:q + 8] == text[q:q + 1] * 8:
                break
            q += 1
        out.append((0, text[p:q], None))
        p = q
    return out


def raw_frame(text: bytes, step=50_000, rle=False, content_size=True, checksum=True, window_log=17, wrong_sum=False, wrong_size=False) -> bytes:
    """One frame of raw (and, with rle, RLE) blocks.  window_log None: a single segment."""
    size = (len(text) + (1 if wrong_size else 0)) if (content_size or window_log is None) else None
    out = [frame_header(size, checksum, window_log)]
    bl = blocks_of(text, min(step, 1 << (window_log or 17)), rle) or [(0, b"", None)]
    for i, (kind, payload, n) in enumerate(bl):
        out.append(block(kind, payload, n, last=i == len(bl) - 1))
    if checksum:
        out.append(struct.pack("<I", (xxh64(text) ^ (1 if wrong_sum else 0)) & 0xffffffff))
    return b"".join(out)


def skippable(payload: bytes = b"between two frames", nibble=7) -> bytes:
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def one_match_block(ml: int, offset: int, last=False) -> bytes:
    """A compressed block of no literals and one sequence -- literal length 0, match length ml (>= 65 539), `offset` (>= 1)
    back --, its three tables of one symbol each (RLE mode)."""
    assert 65_539 <= ml <= 131_072
    ofv = offset + 3
    oc = ofv.bit_length() - 1
    of_extra = ofv - (1 << oc)
    bits = (1 << (oc + 16)) | (of_extra << 16) | (ml - 65_539)   # (from the top: the padding mark, the offset's bits, the match length's)
    stream = bits.to_bytes((oc + 16) // 8 + 1, "little")
    payload = b"\x00" + b"\x01" + b"\x54" + bytes([0, oc, 52]) + stream
    return block(2, payload, last=last)


def run_frame(front: bytes, run: int, back: bytes, checksum=True) -> bytes:
    """front + front[-1] * run + back: the run as ONE match at offset 1 (65 539 <= run <= 131 072)."""
    text = front + front[-1:] * run + back
    parts = [frame_header(len(text), checksum, 17)]
    bl = blocks_of(front, 50_000, False)
    parts += [block(0, p) for _, p, _ in bl]
    parts.append(one_match_block(run, 1))
    bl = blocks_of(back, 50_000, False)
    parts += [block(0, p, last=i == len(bl) - 1) for i, (_, p, _) in enumerate(bl)]
    if checksum:
        parts.append(struct.pack("<I", xxh64(text) & 0xffffffff))
    return b"".join(parts), text


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


def cut_lines(text: bytes, parts: int):
    """`text` in `parts` pieces (cut anywhere)."""
    step = max(1, -(-len(text) // parts))
    return [text[i:i + step] for i in range(0, len(text), step)]


def written_copies(text: bytes) -> dict:
    """The Python-written forms of `text`: {kind: blob}."""
    a, b, c = cut_lines(text, 3)
    return {
        "raw_blocks": raw_frame(text, step=50_000),
        "rle_blocks": raw_frame(text, step=30_000, rle=True),
        "plain_header": raw_frame(text, content_size=False, checksum=False, window_log=20),
        "single_segment": raw_frame(text, checksum=False, window_log=None, step=100_000),
        "frames": raw_frame(a, window_log=None) + raw_frame(b"", checksum=True) + skippable() + raw_frame(b, content_size=False) + raw_frame(c, rle=True),
        "skippable_first": skippable(b"", 0) + raw_frame(text, step=7_000, checksum=False),
    }


def case_workload(grouped: bool, n_records: int):
    """The workload of the gzip tests (config1, seed 31): grouped by name, or shuffled."""
    from slimm_amd.synth import CONFIGS, make_workload
    from tests.test_gpu_bam_decode import _named
    return _named(make_workload(CONFIGS["config1"], seed=31, shuffled=not grouped, n_records=n_records))


def case_text(tmp_dir, grouped: bool, n_records: int) -> bytes:
    """... and its SAM text."""
    from tests.bam_io import write_sam
    w = case_workload(grouped, n_records)
    p = os.path.join(str(tmp_dir), f"case_{int(grouped)}_{n_records}.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    return open(p, "rb").read()
