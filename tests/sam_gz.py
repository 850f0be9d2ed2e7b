"""Compressed copies of a SAM file for the reader and command tests: plain gzip (one member, several members, the system's
gzip tool) and BGZF (tests/bam_io._bgzf_block) with blocks cut anywhere -- inside lines, a header over several blocks.
Test infrastructure only."""
import gzip
import os
import random
import shutil
import subprocess

from tests.bam_io import _bgzf_block

GZIP_TOOL = shutil.which("gzip")
BGZF_EOF = _bgzf_block(b"")


def header_len(text: bytes) -> int:
    """Bytes of the header: everything in front of the first alignment line (lines before it that are empty or start with
    '@')."""
    off = 0
    for line in text.splitlines(keepends=True):
        if line.strip(b"\r\n") and not line.startswith(b"@"):
            break
        off += len(line)
    return off


def bgzf(text: bytes, seed: int = 0, header_blocks: int = 3, lo: int = 1, hi: int = 60_000, eof: bool = True) -> bytes:
    """BGZF blocks of `text`: the header cut into `header_blocks` blocks (or more), the rest into blocks of lo..hi bytes
    at random places (inside lines); hi <= 65,536."""
    rng = random.Random(seed)
    h = header_len(text)
    cuts = [0]
    if h:
        step = max(1, min(h // header_blocks - 1, 65_280))   # (a block holds at most 64 KiB)
        cuts += list(range(step, h, step))
    p = cuts[-1]
    while p < len(text):
        p = min(len(text), max(p + 1, p + rng.randint(lo, hi)))
        cuts.append(p)
    if cuts[-1] != len(text):
        cuts.append(len(text))
    blocks = [_bgzf_block(text[a:b]) for a, b in zip(cuts, cuts[1:]) if b > a]
    return b"".join(blocks) + (BGZF_EOF if eof else b"")


def gzip_members(text: bytes, parts: int = 1) -> bytes:
    """`text` as `parts` gzip members back to back (Python's gzip)."""
    step = max(1, -(-len(text) // parts))
    return b"".join(gzip.compress(text[i:i + step]) for i in range(0, len(text), step)) or gzip.compress(b"")


def gzip_tool(path: str, out: str) -> None:
    """`gzip -c path > out` with the system's tool."""
    with open(out, "wb") as f:
        subprocess.run([GZIP_TOOL, "-c", path], stdout=f, check=True)


def compressed_copies(sam_path: str, outdir: str, seed: int = 0):
    """{kind: path} of the compressed copies of a SAM file: gzip (Python), gzip2 (two members), bgzf; gzip_tool where the
    system has gzip."""
    text = open(sam_path, "rb").read()
    stem = os.path.join(outdir, os.path.basename(sam_path))
    out = {}
    for kind, blob in (("gzip", gzip_members(text)), ("gzip2", gzip_members(text, 2)), ("bgzf", bgzf(text, seed=seed))):
        p = f"{stem}.{kind}.gz"
        open(p, "wb").write(blob)
        out[kind] = p
    if GZIP_TOOL:
        out["gzip_tool"] = f"{stem}.tool.gz"
        gzip_tool(sam_path, out["gzip_tool"])
    return out
