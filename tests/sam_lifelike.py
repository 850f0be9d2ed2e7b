"""SAM text and BAM records as a mapper writes them, for the device decoders' tests: the records of a workload -- names,
flags, references and positions as tests/bam_io.write_sam writes them, under the same header -- with sequences over ACGT of
1 .. 300 bases, Phred-like quality strings, a CIGAR of the sequence's length and two or three tags.  write_sam's text is
almost all long matches for every compressor (SEQ = A..., QUAL = *); this one is mostly literals, which is what the
decoders' literal paths need.  Everything is drawn from random.Random(seed), so that the text is the same on every machine
(tests/test_lifelike_inputs.py pins one sha256).  Test infrastructure only."""
import random
import types

import numpy as np

from slimm_amd.workload import Records
from tests.bam_io import _bgzf_block, _file_flags, bam_header_bytes, bam_record_bytes, qnames_of, sam_header, write_sam

BASES, BASE_WEIGHTS = "ACGTN", (99, 99, 99, 99, 4)   # (about 1 % N)


def _cigar(rng, n: int) -> str:
    """Operations whose query-consuming lengths (S, M, I) add up to n; a deletion consumes none."""
    if n < 8 or rng.random() < 0.6:
        return f"{n}M"
    clip = rng.randrange(1, n // 4 + 1) if rng.random() < 0.4 else 0
    ins = rng.randrange(1, 4) if rng.random() < 0.5 else 0
    rest = n - clip - ins
    a = rng.randrange(1, rest)
    mid = f"{ins}I" if ins else f"{rng.randrange(1, 30)}D"
    return (f"{clip}S" if clip else "") + f"{a}M{mid}{rest - a}M"


def _md(rng, n: int, nm: int) -> str:
    """An MD string of nm mismatches over n bases."""
    cuts = sorted(rng.randrange(n) for _ in range(nm))
    out, at = [], 0
    for c in cuts:
        out.append(f"{max(c - at, 0)}{BASES[rng.randrange(4)]}")
        at = c + 1
    return "".join(out) + str(max(n - at, 0))


def lifelike_text(w, seed: int, hi_bytes: bool = False) -> bytes:
    """The SAM text of workload `w`.  Record 3 has a sequence of one base, record 7 of two; about one record in a hundred has
    SEQ and QUAL `*`.  hi_bytes: every record also carries a Z tag of 0 .. 40 bytes from 128 .. 255."""
    rng = random.Random(seed)
    rec = w.records
    q, fflag = qnames_of(rec), _file_flags(rec)
    out = [sam_header(w.ref_names, w.ref_len).encode()]
    for i in range(len(rec)):
        r = int(rec.ref_id[i])
        rn = w.ref_names[r] if r >= 0 else "*"
        n = 1 if i == 3 else 2 if i == 7 else 0 if rng.random() < 0.01 else rng.randrange(1, 301)
        if n:
            seq = "".join(rng.choices(BASES, weights=BASE_WEIGHTS, k=n))
            qual = "".join(chr(min(126, max(33, round(rng.gauss(68, 14))))) for _ in range(n))
            cigar = _cigar(rng, n)
        else:
            seq = qual = cigar = "*"
        nm = rng.randrange(n // 12 + 1)
        tags = [f"NM:i:{nm}", f"MD:Z:{_md(rng, max(n, 1), nm)}"] + ([f"AS:i:{rng.randrange(2 * n + 1)}"] if rng.random() < 0.6 else [])
        line = f"{q[i]}\t{int(fflag[i])}\t{rn}\t{int(rec.begin_pos[i]) + 1}\t{rng.randrange(61)}\t{cigar}\t*\t0\t0\t{seq}\t{qual}\t" + "\t".join(tags)
        line = line.encode()
        if hi_bytes:
            line += b"\tXB:Z:" + bytes(rng.randrange(128, 256) for _ in range(rng.randrange(41)))
        out.append(line + b"\n")
    return b"".join(out)


def plain_text(w) -> bytes:
    """write_sam's text of the same workload: the text the other codec tests decode."""
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_sam(os.path.join(d, "w.sam"), w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
        return open(os.path.join(d, "w.sam"), "rb").read()


def lifelike_bam(w, seed: int, lo: int = 500, hi: int = 65_000):
    """(BGZF blocks of a BAM file of `w` with lifelike records, cut at lo .. hi inflated bytes; the inflated bytes in
    front of the first record; the records' bytes)."""
    head = bam_header_bytes(w.ref_names, w.ref_len)
    body = bam_record_bytes(w.records, lifelike_seed=seed)
    data, rng, p, blocks = head + body, random.Random(seed), 0, []
    first = min(65_000, len(head) + rng.randint(lo, min(hi, 20_000)))   # (the header and the first records in one block)
    while p < len(data):
        e = min(len(data), p + (first if p == 0 else rng.randint(lo, hi)))
        blocks.append(_bgzf_block(data[p:e]))
        p = e
    return b"".join(blocks) + _bgzf_block(b""), len(head), body


def small_workload(records: int = 350):
    """`records` records of 120 reads on the four references the program configures (R0 .. R3, 5 000 bases), grouped by name; a few
    unmapped."""
    rng = np.random.default_rng(5)
    read = np.sort(rng.integers(0, 120, size=records))
    flag = np.where(rng.random(records) < 0.5, 0x40, 0x80).astype(np.uint16)
    ref = rng.integers(0, 4, size=records).astype(np.int32)
    ref[::37] = -1
    flag[::37] |= 4
    rec = Records(read.astype(np.uint64), flag, ref, rng.integers(0, 4_700, size=records).astype(np.int32), [f"read/{i}/" for i in read.tolist()])
    return types.SimpleNamespace(ref_names=["R0", "R1", "R2", "R3"], ref_len=[5_000] * 4, records=rec)


# ---- compressed copies, made with the standard library -------------------------------------------------------------------
def cut_at_lines(text: bytes, parts: int):
    """`text` in `parts` pieces of about equal size, each ending with a line."""
    out, at = [], 0
    for k in range(1, parts):
        end = text.index(b"\n", max(at, k * len(text) // parts)) + 1
        out.append(text[at:end])
        at = end
    return out + [text[at:]]


def xz_copies(text: bytes) -> dict:
    """{kind: blob}: preset 6 with CRC64; a 4 KiB dictionary with lc 4, lp 0, pb 0 and CRC32; preset 9 with lc 0, lp 4, pb 4; no
    check; three streams back to back."""
    import lzma
    lz = lzma.FILTER_LZMA2
    return {
        "preset6": lzma.compress(text, check=lzma.CHECK_CRC64, preset=6),
        "lc4_dict4k": lzma.compress(text, check=lzma.CHECK_CRC32, filters=[{"id": lz, "preset": 1, "lc": 4, "lp": 0, "pb": 0, "dict_size": 4096}]),
        "lc0lp4pb4": lzma.compress(text, check=lzma.CHECK_CRC64, filters=[{"id": lz, "preset": 9, "lc": 0, "lp": 4, "pb": 4}]),
        "none": lzma.compress(text, check=lzma.CHECK_NONE, preset=6),
        "three_streams": b"".join(lzma.compress(p, check=lzma.CHECK_CRC64, preset=6) for p in cut_at_lines(text, 3)),
    }


GZIP_KINDS = {"level6": (6, 8, "Z_DEFAULT_STRATEGY"), "mem1": (1, 1, "Z_DEFAULT_STRATEGY"), "huffman": (6, 8, "Z_HUFFMAN_ONLY"),
              "rle": (6, 8, "Z_RLE"), "fixed": (6, 8, "Z_FIXED")}


def gzip_member(text: bytes, kind: str) -> bytes:
    import zlib
    level, mem, strategy = GZIP_KINDS[kind]
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, getattr(zlib, strategy))
    return c.compress(text) + c.flush()


def gzip_copies(text: bytes) -> dict:
    """{kind: [members]}: level 6; level 1 at memLevel 1; Huffman codes only; Z_RLE; Z_FIXED; two members back to back."""
    out = {k: [gzip_member(text, k)] for k in GZIP_KINDS}
    out["two_members"] = [gzip_member(p, "level6") for p in cut_at_lines(text, 2)]
    return out


def bzip2_copies(text: bytes) -> dict:
    """{kind: blob}: level 1, level 9, two streams back to back."""
    import bz2
    a, b = cut_at_lines(text, 2)
    return {"level1": bz2.compress(text, 1), "level9": bz2.compress(text, 9), "two_streams": bz2.compress(a, 9) + bz2.compress(b, 1)}


# ---- the committed zstd inputs (tests/golden/zstd_lifelike, made by make_inputs.py there) ----------------------------------
ZSTD_RECORDS, ZSTD_SEED = 300, 31
# kind -> (file, hi_bytes, level, window_log, content size and checksum)
ZSTD_KINDS = {"l1": ("lifelike_grouped_l1.sam.zst", False, 1, 0, True), "l19": ("lifelike_grouped_l19_hi.sam.zst", True, 19, 0, True),
              "wlog10": ("lifelike_grouped_wlog10.sam.zst", False, 3, 10, True), "plain": ("lifelike_grouped_plain_hi.sam.zst", True, 3, 0, False)}


def zstd_golden(kind: str) -> bytes:
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_lifelike", ZSTD_KINDS[kind][0]), "rb").read()


def zstd_text(kind: str) -> bytes:
    """The text of a committed zstd input, from its seed."""
    from tests.sam_zst import case_workload
    return lifelike_text(case_workload(True, ZSTD_RECORDS), ZSTD_SEED, hi_bytes=ZSTD_KINDS[kind][1])
