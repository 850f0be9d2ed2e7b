"""lzip copies of a SAM text for the reader, command and device tests.  A member is written with Python's `lzma`: a raw LZMA1
stream with lc 3, lp 0, pb 2 always ends in the End Of Stream marker, and an LZMADecompressor of the same filter reports
`eof` at the marker and leaves the 20 trailer bytes in `unused_data` -- that decoder is the tests' reference.  Also: the
committed inputs (tests/golden/lzip, made by make_inputs.py there: liblzma's output differs between versions), a forward and
a backward walker in plain Python, the census under the names of Slimm.lzip_stats(), and the damage cases.  No test needs an
`lzip` or `plzip` binary.  Test infrastructure only."""
import lzma
import os
import struct
import zlib

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)
from tests.sam_zst import case_text, case_workload, cut_lines  # noqa: F401  (the texts are the zstd tests')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzip")
MAGIC = b"LZIP"
HEADER, TRAILER, MEMBER_MIN = 6, 20, 6 + 5 + 20
# the committed inputs: kind -> (records of the config1 text, file name with the order's tag, orders committed)
GOLDEN_KINDS = {
    "m17": (3_000, "config1_{}_m17.sam.lz", ("grouped", "any")),
    "one": (1_000, "short_{}_one.sam.lz", ("grouped",)),
    "d4k": (1_000, "short_{}_d4k.sam.lz", ("grouped",)),
    "empty_between": (1_000, "short_{}_empty_between.sam.lz", ("any",)),
}


def dict_size_of(ds: int) -> int:
    """The DS byte's size; 0: not a legal one."""
    bits = ds & 31
    if not 12 <= bits <= 29:
        return 0
    size = (1 << bits) - ((1 << bits) // 16) * (ds >> 5)
    return size if 4096 <= size <= 1 << 29 else 0


def ds_byte_of(size: int) -> int:
    """The smallest legal dictionary that holds `size`, as a DS byte."""
    best = None
    for ds in range(256):
        d = dict_size_of(ds)
        if d >= size and (best is None or d < best[0]):
            best = (d, ds)
    return best[1]


def _filters(dict_size):
    return [{"id": lzma.FILTER_LZMA1, "dict_size": dict_size, "lc": 3, "lp": 0, "pb": 2}]


def wrap(stream: bytes, text: bytes, ds: int, version=1) -> bytes:
    """A member around an LZMA stream that decodes to `text`."""
    return MAGIC + bytes([version, ds]) + stream + struct.pack("<IQQ", zlib.crc32(text), len(text), HEADER + len(stream) + TRAILER)


def member(text: bytes, dict_size=1 << 16) -> bytes:
    ds = ds_byte_of(dict_size)
    return wrap(lzma.compress(text, format=lzma.FORMAT_RAW, filters=_filters(dict_size_of(ds))), text, ds)


def members(text: bytes, step: int, dict_size=1 << 16) -> bytes:
    """Members of `step` bytes of text each, as `plzip` cuts its input (there: twice the dictionary size)."""
    return b"".join(member(text[i:i + step], dict_size) for i in range(0, len(text), step)) if text else member(b"", dict_size)


# ---- the walkers
def legal_header(b: bytes, q: int) -> bool:
    return b[q:q + 4] == MAGIC and len(b) >= q + 6 and b[q + 4] == 1 and dict_size_of(b[q + 5]) > 0


def walk(blob: bytes):
    """Forward, as the format's finder: [{"at", "size", "ds", "dict_size", "crc", "data_size", "stream_at", "trailer_at"}]."""
    out, s = [], 0
    while s < len(blob):
        assert legal_header(blob, s), s
        q = s + MEMBER_MIN
        while True:
            assert q <= len(blob), ("no end", s)
            if (q == len(blob) or legal_header(blob, q)) and struct.unpack_from("<Q", blob, q - 8)[0] == q - s:
                break
            q += 1
        crc, data_size, _ = struct.unpack_from("<IQQ", blob, q - TRAILER)
        out.append({"at": s, "size": q - s, "ds": blob[s + 5], "dict_size": dict_size_of(blob[s + 5]), "crc": crc, "data_size": data_size,
                    "stream_at": s + HEADER, "trailer_at": q - TRAILER})
        s = q
    return out


def walk_back(blob: bytes):
    """Backward over the member_size fields: [(at, member_size, data_size)] in file order; None when the chain does not close on byte 0."""
    out, end = [], len(blob)
    while end > 0:
        if end < MEMBER_MIN:
            return None
        _, data_size, size = struct.unpack_from("<IQQ", blob, end - TRAILER)
        if size < MEMBER_MIN or size > end or not legal_header(blob, end - size):
            return None
        out.append((end - size, size, data_size))
        end -= size
    return out[::-1] or None


def decode_member(blob: bytes, m: dict) -> bytes:
    """The reference: Python's raw decoder on the member's stream; the marker must stand at the trailer, the trailer must fit."""
    d = lzma.LZMADecompressor(format=lzma.FORMAT_RAW, filters=_filters(m["dict_size"]))
    text = d.decompress(blob[m["stream_at"]:m["at"] + m["size"]])
    assert d.eof and len(d.unused_data) == TRAILER, (d.eof, len(d.unused_data))
    assert len(text) == m["data_size"] and zlib.crc32(text) == m["crc"], "trailer"
    return text


def decode(blob: bytes) -> bytes:
    return b"".join(decode_member(blob, m) for m in walk(blob))


def refused_by_reference(blob: bytes) -> bool:
    """Does the reference refuse `blob` -- the walk, Python's decoder, or the trailer comparison?"""
    try:
        decode(blob)
    except (AssertionError, lzma.LZMAError, EOFError, struct.error, IndexError):
        return True
    return False


def census(blob: bytes) -> dict:
    """What `blob` holds, by the walker, under the names of Slimm.lzip_stats() (match bytes and distances: not known here)."""
    ms = walk(blob)
    return {"members": len(ms), "empty_members": sum(1 for m in ms if not m["data_size"]), "crc32_checked": len(ms),
            "max_dict": max(m["dict_size"] for m in ms), "text_bytes": sum(m["data_size"] for m in ms), "compressed_bytes": len(blob)}


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


def written_copies(text: bytes) -> dict:
    """Forms of the short text written here, with this machine's liblzma: {kind: blob}."""
    parts = cut_lines(text, 3)
    return {
        "three_members": b"".join(member(p) for p in parts),
        "empty_first_and_last": member(b"") + member(text, 1 << 20) + member(b""),
        "every_fraction": b"".join(wrap(lzma.compress(p, format=lzma.FORMAT_RAW, filters=_filters(dict_size_of((f << 5) | 17))), p, (f << 5) | 17)
                                   for f, p in enumerate(cut_lines(text, 8))),
    }


# ---- damage
def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def with_bytes(blob, at, v: bytes):
    return blob[:at] + v + blob[at + len(v):]


def damaged(text: bytes):
    """(the good three-member file, {name: (bytes, the cause's words)}): cut behind every structural element and damaged in
    every kind of place."""
    blob = written_copies(text)["three_members"]
    m0, m1, m2 = walk(blob)
    return blob, {
        "inside_the_magic": (blob[:3], "member at byte 0: truncated"),
        "inside_the_header": (blob[:5], "member at byte 0: truncated"),
        "inside_the_stream": (blob[:m0["stream_at"] + 100], "member at byte 0: truncated"),
        "inside_the_trailer": (blob[:m0["trailer_at"] + 7], "member at byte 0: truncated"),
        "inside_the_second_member": (blob[:m1["at"] + m1["size"] // 2], f"member at byte {m1['at']}: truncated"),
        "inside_the_last_trailer": (blob[:-1], f"member at byte {m2['at']}: truncated"),
        "trailing_data": (blob + b"garbage!", f"at byte {len(blob)}: trailing data behind the last lzip member"),
        "trailing_short": (blob + b"\n", f"at byte {len(blob)}: trailing data behind the last lzip member"),
        "version_0": (with_bytes(blob, 4, b"\x00"), "member at byte 0: lzip version 0"),
        "version_2": (with_bytes(blob, 4, b"\x02"), "member at byte 0: an lzip version other than 1"),
        "dictionary_too_small": (with_bytes(blob, 5, b"\x0b"), "member at byte 0: a dictionary size below 4 KiB or above 512 MiB"),
        "dictionary_too_large": (with_bytes(blob, 5, b"\x1e"), "member at byte 0: a dictionary size below 4 KiB or above 512 MiB"),
        "crc": (flipped(blob, m1["trailer_at"]), f"member at byte {m1['at']}: CRC32 mismatch"),
        "lzma_data": (flipped(blob, m1["stream_at"] + 40), f"member at byte {m1['at']}: "),
        "data_size_one_more": (with_bytes(blob, m0["trailer_at"] + 4, struct.pack("<Q", m0["data_size"] + 1)), "member at byte 0: an end marker in front of the member's data_size"),
        "data_size_one_less": (with_bytes(blob, m0["trailer_at"] + 4, struct.pack("<Q", m0["data_size"] - 1)), "member at byte 0: "),
        "data_size_absurd": (with_bytes(blob, m0["trailer_at"] + 4, struct.pack("<Q", 1 << 50)), "member at byte 0: an end marker in front of the member's data_size"),
        "first_range_byte": (with_bytes(blob, m0["stream_at"], b"\x01"), "member at byte 0: a range coder that does not start with a zero byte"),
        "not_lzip": (b"@HD\tVN:1.0\n" * 8, "member at byte 0: bytes that start no lzip member"),
    }


TRUNCATED = ["inside_the_magic", "inside_the_header", "inside_the_stream", "inside_the_trailer", "inside_the_second_member", "inside_the_last_trailer"]
DAMAGE = TRUNCATED + ["trailing_data", "trailing_short", "version_0", "version_2", "dictionary_too_small", "dictionary_too_large", "crc", "lzma_data",
                      "data_size_one_more", "data_size_one_less", "data_size_absurd", "first_range_byte", "not_lzip"]
