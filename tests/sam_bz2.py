"""bzip2-compressed copies of a SAM text for the reader, ABI and command tests, made with Python's bz2 module: one stream at
level 1 or 9, many streams back to back of different levels with an empty one among them (as pbzip2 / lbzip2 write), a
header over several blocks; and ways to damage one.  Larger inputs are compressed one stream per chunk in a process
pool.  Test infrastructure only."""
import bz2
import os
from concurrent.futures import ProcessPoolExecutor

from tests.sam_gz import header_len  # noqa: F401  (re-exported: the tests' skip)

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090


def one_stream(text: bytes, level: int = 9) -> bytes:
    return bz2.compress(text, level)


def _compress(args):
    chunk, level = args
    return bz2.compress(chunk, level)


def streams(text: bytes, chunk: int = 200_000, levels=(1, 9, 5, 2), empty_at: int = 1, workers: int = 0) -> bytes:
    """`text` as one stream per `chunk` bytes, back to back, levels in turn; an empty stream in front of the empty_at-th
    chunk (-1: none).  workers > 0: a process pool."""
    jobs = [(text[i:i + chunk], levels[(i // chunk) % len(levels)]) for i in range(0, len(text), chunk)] or [(b"", 9)]
    if 0 <= empty_at <= len(jobs):
        jobs.insert(empty_at, (b"", 3))
    if workers > 0:
        with ProcessPoolExecutor(max_workers=workers) as ex:
            return b"".join(ex.map(_compress, jobs, chunksize=4))
    return b"".join(_compress(j) for j in jobs)


def header_spanning(text: bytes, level: int = 1) -> bytes:
    """A copy whose header lies in several blocks: the header as streams of a few hundred bytes each, the rest one stream."""
    h = header_len(text)
    step = max(1, h // 4)
    return b"".join(bz2.compress(text[i:min(h, i + step)], level) for i in range(0, h, step)) + bz2.compress(text[h:], level)


def copies(text: bytes):
    """{kind: blob}: the copies every reader test goes through."""
    return {
        "level1": one_stream(text, 1),
        "level9": one_stream(text, 9),
        "streams": streams(text, chunk=max(1, len(text) // 7 + 1)),
        "header_blocks": header_spanning(text),
    }


def write_copies(sam_path: str, outdir: str):
    """{kind: path} of the bzip2 copies of a SAM file."""
    text = open(sam_path, "rb").read()
    stem = os.path.join(outdir, os.path.basename(sam_path))
    out = {}
    for kind, blob in copies(text).items():
        out[kind] = f"{stem}.{kind}.bz2"
        open(out[kind], "wb").write(blob)
    return out


# ---- finding and damaging blocks -----------------------------------------------------------------------------------------
def _bits(blob: bytes) -> int:
    return int.from_bytes(blob, "big")


def magics(blob: bytes, magic: int = BLOCK_MAGIC):
    """Bit offsets at which the 48-bit `magic` stands (blocks, or end-of-stream markers), in order."""
    import numpy as np
    bits = np.unpackbits(np.frombuffer(blob, dtype=np.uint8))
    pat = magic.to_bytes(6, "big")
    out = []
    for k in range(8):
        shifted = np.packbits(bits[k:]).tobytes()
        p = shifted.find(pat)
        while p >= 0:
            out.append(p * 8 + k)
            p = shifted.find(pat, p + 1)
    return sorted(out)


def set_bits(blob: bytes, bit: int, width: int, value: int) -> bytes:
    """`width` bits at bit offset `bit` (MSB first) replaced by `value`."""
    n = len(blob) * 8
    v = _bits(blob)
    shift = n - bit - width
    v = (v & ~(((1 << width) - 1) << shift)) | ((value & ((1 << width) - 1)) << shift)
    return v.to_bytes(len(blob), "big")


def get_bits(blob: bytes, bit: int, width: int) -> int:
    n = len(blob) * 8
    return (_bits(blob) >> (n - bit - width)) & ((1 << width) - 1)


def flip_bit(blob: bytes, bit: int) -> bytes:
    return set_bits(blob, bit, 1, get_bits(blob, bit, 1) ^ 1)
