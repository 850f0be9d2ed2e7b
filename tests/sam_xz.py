"""xz copies of a SAM text for the reader, command and device tests: the committed compressor-made inputs (tests/golden/xz,
made by make_inputs.py there with `xz` 5.2.5); a pure-Python walker of streams, blocks, LZMA2 chunks and indexes, with its
own CRC64 table, by which tests state what their inputs contain and where to damage them; and writers of containers in plain
Python for what the compressor does not emit on SAM text -- blocks of uncompressed chunks only, compressor-made blocks
wrapped again into other streams, streams back to back with stream padding, an empty stream.  No test needs an `xz` binary
or liblzma.  Test infrastructure only."""
import os
import struct
import zlib

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)
from tests.sam_zst import case_text, case_workload, cut_lines  # noqa: F401  (the texts are the zstd tests')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xz")
MAGIC, FOOTER_MAGIC = b"\xfd7zXZ\x00", b"YZ"
CHECK_BYTES = {0: 0, 1: 4, 4: 8, 10: 32}
# the committed inputs: kind -> (records of the config1 text, file name with the order's tag)
GOLDEN_KINDS = {
    "mt": (3_000, "config1_{}_mt.sam.xz"), "blocks": (3_000, "config1_{}_blocks.sam.xz"), "one": (15_000, "long_{}_one.sam.xz"),
    "l0": (1_000, "short_{}_l0.sam.xz"), "l9e": (1_000, "short_{}_l9e.sam.xz"), "lc0lp2": (1_000, "short_{}_lc0lp2.sam.xz"),
    "lc4": (1_000, "short_{}_lc4.sam.xz"), "none": (1_000, "short_{}_none.sam.xz"), "sha256": (1_000, "short_{}_sha256.sam.xz"),
}
REFUSED_KIND = (1_000, "short_{}_bcj.sam.xz")   # --x86 --lzma2: to be refused
PARTS = (1_000, "short_{}_part{}.sam.xz")       # the short text in three pieces (cut_lines), each compressed by itself


# ---- CRC64 (ECMA-182, reflected)
def _crc64_table():
    out = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0xC96C5795D7870F42 if c & 1 else c >> 1
        out.append(c)
    return out


_T64 = _crc64_table()


def crc64(data: bytes) -> int:
    c = (1 << 64) - 1
    for b in data:
        c = _T64[(c ^ b) & 0xff] ^ (c >> 8)
    return c ^ ((1 << 64) - 1)


def check_of(kind: int, text: bytes) -> bytes:
    if kind == 1:
        return struct.pack("<I", zlib.crc32(text))
    if kind == 4:
        return struct.pack("<Q", crc64(text))
    if kind == 10:
        import hashlib
        return hashlib.sha256(text).digest()
    return b""


# ---- the walker
def _vli(b: bytes, p: int):
    v = 0
    for i in range(9):
        v |= (b[p] & 0x7f) << (7 * i)
        p += 1
        if not b[p - 1] & 0x80:
            return v, p
    raise AssertionError("bad multibyte integer")


def walk_chunks(b: bytes, p: int):
    """The LZMA2 chunks from b[p] on: ([{"at", "control", "usize", "csize", "header", "props"}], the byte behind the end marker)."""
    out = []
    while b[p]:
        c = b[p]
        if c >= 0x80:
            ch = {"at": p, "control": c, "usize": (((c & 0x1f) << 16) | (b[p + 1] << 8) | b[p + 2]) + 1, "csize": ((b[p + 3] << 8) | b[p + 4]) + 1,
                  "header": 6 if c >= 0xc0 else 5, "props": b[p + 5] if c >= 0xc0 else None}
        else:
            assert c <= 2, (p, c)
            n = ((b[p + 1] << 8) | b[p + 2]) + 1
            ch = {"at": p, "control": c, "usize": n, "csize": n, "header": 3, "props": None}
        out.append(ch)
        p += ch["header"] + ch["csize"]
    return out, p + 1


def walk(blob: bytes):
    """The streams of `blob`: [{"at", "check", "blocks": [{"at", "header", "filters", "sizes" (stated in the header: compressed,
    uncompressed, None where not), "data_at", "chunks", "text", "pad_at", "check_at", "unpadded"}], "index_at", "records",
    "footer_at", "end", "padding" (zero bytes behind it)}]."""
    streams, p = [], 0
    while p < len(blob):
        assert blob[p:p + 6] == MAGIC, p
        assert zlib.crc32(blob[p + 6:p + 8]) == struct.unpack_from("<I", blob, p + 8)[0]
        s = {"at": p, "check": blob[p + 7], "blocks": []}
        p += 12
        while blob[p]:
            hb = (blob[p] + 1) * 4
            assert zlib.crc32(blob[p:p + hb - 4]) == struct.unpack_from("<I", blob, p + hb - 4)[0]
            flags, q = blob[p + 1], p + 2
            sizes = [None, None]
            if flags & 0x40:
                sizes[0], q = _vli(blob, q)
            if flags & 0x80:
                sizes[1], q = _vli(blob, q)
            filters = []
            for _ in range((flags & 3) + 1):
                fid, q = _vli(blob, q)
                n, q = _vli(blob, q)
                filters.append((fid, blob[q:q + n]))
                q += n
            blk = {"at": p, "header": hb, "filters": filters, "sizes": tuple(sizes), "data_at": p + hb}
            if [f for f, _ in filters] != [0x21]:   # (not LZMA2 alone: its data is not walked)
                blk["chunks"], end = [], p + hb + sizes[0] if sizes[0] is not None else None
                assert end is not None
            else:
                blk["chunks"], end = walk_chunks(blob, p + hb)
            blk["text"] = sum(c["usize"] for c in blk["chunks"])
            blk["pad_at"] = end
            blk["check_at"] = end + (-(end - p) % 4)
            blk["unpadded"] = end - p + CHECK_BYTES[s["check"]]
            s["blocks"].append(blk)
            p = blk["check_at"] + CHECK_BYTES[s["check"]]
        s["index_at"] = p
        n, q = _vli(blob, p + 1)
        s["records"] = []
        for _ in range(n):
            a, q = _vli(blob, q)
            u, q = _vli(blob, q)
            s["records"].append((a, u))
        q += -(q - p) % 4
        assert zlib.crc32(blob[p:q]) == struct.unpack_from("<I", blob, q)[0]
        s["footer_at"] = q + 4
        p = q + 16
        assert blob[p - 2:p] == FOOTER_MAGIC
        s["end"] = p
        while p + 4 <= len(blob) and blob[p:p + 4] == bytes(4):
            p += 4
        s["padding"] = p - s["end"]
        streams.append(s)
    return streams


def census(blob: bytes) -> dict:
    """What `blob` holds, by the walker, under the names of Slimm.xz_stats()."""
    out = {k: 0 for k in ("streams", "blocks", "lzma_chunks", "raw_chunks", "state_resets", "prop_changes", "odd_props", "check_none", "check_crc32",
                          "check_crc64", "sha256_unverified", "text", "index_records")}
    out["compressed"] = len(blob)
    for s in walk(blob):
        out["streams"] += 1
        out["index_records"] += len(s["records"])
        for b in s["blocks"]:
            out["blocks"] += 1
            out[{0: "check_none", 1: "check_crc32", 4: "check_crc64", 10: "sha256_unverified"}[s["check"]]] += 1
            out["text"] += b["text"]
            for c in b["chunks"]:
                out["lzma_chunks" if c["control"] >= 0x80 else "raw_chunks"] += 1
                out["state_resets"] += c["control"] >= 0xa0
                out["prop_changes"] += c["control"] >= 0xc0
                out["odd_props"] += c["control"] >= 0xc0 and c["props"] != 0x5d
    return out


# ---- the writers
def _vli_bytes(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def stream_header(check: int) -> bytes:
    flags = bytes([0, check])
    return MAGIC + flags + struct.pack("<I", zlib.crc32(flags))


def block_header(dict_byte=0x16, sizes=(None, None), filters=None) -> bytes:
    """One filter (LZMA2 with that dictionary byte) unless `filters` [(id, properties)] says otherwise."""
    filters = filters if filters is not None else [(0x21, bytes([dict_byte]))]
    body = bytes([(len(filters) - 1) | (0x40 if sizes[0] is not None else 0) | (0x80 if sizes[1] is not None else 0)])
    for v in sizes:
        if v is not None:
            body += _vli_bytes(v)
    for fid, props in filters:
        body += _vli_bytes(fid) + _vli_bytes(len(props)) + props
    total = -(-(1 + len(body) + 4) // 4) * 4
    head = bytes([total // 4 - 1]) + body + bytes(total - 4 - 1 - len(body))
    return head + struct.pack("<I", zlib.crc32(head))


def index_of(records) -> bytes:
    body = b"\x00" + _vli_bytes(len(records)) + b"".join(_vli_bytes(a) + _vli_bytes(u) for a, u in records)
    body += bytes(-len(body) % 4)
    return body + struct.pack("<I", zlib.crc32(body))


def stream_footer(check: int, index_bytes: int) -> bytes:
    body = struct.pack("<I", index_bytes // 4 - 1) + bytes([0, check])
    return struct.pack("<I", zlib.crc32(body)) + body + FOOTER_MAGIC


def stream_of(blocks, check=4) -> bytes:
    """A stream of `blocks` [(header bytes, LZMA2 data with its end marker, text)], checks of kind `check`, the index rebuilt."""
    out, records = [stream_header(check)], []
    for head, data, text in blocks:
        out += [head, data, bytes(-(len(head) + len(data)) % 4), check_of(check, text)]
        records.append((len(head) + len(data) + CHECK_BYTES[check], len(text)))
    index = index_of(records)
    return b"".join(out) + index + stream_footer(check, len(index))


def raw_chunks(text: bytes, step=50_000, first_control=1) -> bytes:
    """LZMA2 data of uncompressed chunks of at most `step` (<= 65 536) bytes, the first with the dictionary reset."""
    out = []
    for i in range(0, len(text), step):
        part = text[i:i + step]
        out.append(bytes([first_control if i == 0 else 2]) + struct.pack(">H", len(part) - 1) + part)
    return b"".join(out) + b"\x00"


def stored_chunks(text: bytes, step=50_000, check=4, blocks=1, sizes=False) -> bytes:
    """One stream whose blocks hold uncompressed chunks only."""
    parts = cut_lines(text, blocks) if text else [b""]
    made = []
    for part in parts:
        data = raw_chunks(part, step)
        made.append((block_header(sizes=(len(data), len(part)) if sizes else (None, None)), data, part))
    return stream_of(made, check)


def blocks_of(blob: bytes, texts):
    """The blocks of a compressor-made `blob` for stream_of: (header, data, text) each; texts: the blocks' texts in order."""
    out = []
    for b, text in zip((b for s in walk(blob) for b in s["blocks"]), texts):
        assert b["text"] == len(text)
        out.append((blob[b["at"]:b["data_at"]], blob[b["data_at"]:b["pad_at"]], text))
    return out


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


def part_blocks(text: bytes, tag: str):
    """The three single-block compressor outputs of the short text's pieces, as blocks."""
    pieces = cut_lines(text, 3)
    return [blocks_of(golden(PARTS[1].format(tag, i)), [pieces[i]])[0] for i in range(3)]


def written_copies(text: bytes, tag: str) -> dict:
    """The Python-written forms of the short text (1 000 records; tag: "grouped" / "any"): {kind: blob}."""
    parts = part_blocks(text, tag)
    real = stream_of(parts, check=1)
    return {
        "stored_chunks": stored_chunks(text, step=40_000, check=4, blocks=2, sizes=True),
        "reblocked": real,
        "two_streams_padded": stream_of(parts[:1], check=4) + bytes(8) + stream_of(parts[1:], check=1) + bytes(4),
        "empty_stream": stream_of([], check=4) + real,
    }
