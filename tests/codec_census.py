"""The census of what the committed xz and zstd inputs reach: tests/lzma_paths.py and tests/zstd_paths.py over every file of
tests/golden/xz, zstd, zstd_frames and zstd_lifelike and over the xz copies tests/sam_lifelike.py makes.
tests/golden/codec_paths/make_census.py writes it to committed_inputs.json there; tests/test_codec_paths.py compares.  Test
infrastructure only."""
import glob
import os
from collections import Counter

from tests import lzma_paths, zstd_paths

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
JSON = os.path.join(GOLDEN, "codec_paths", "committed_inputs.json")


def xz_files():
    """{name: bytes}: the committed files (the x86-filtered one is to be refused: not decoded) and the lifelike copies."""
    out = {os.path.relpath(p, GOLDEN): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(GOLDEN, "xz", "*.xz"))) if "_bcj" not in p}
    from tests import sam_lifelike as L
    text = L.lifelike_text(L.small_workload(), 5, hi_bytes=True)
    out.update({f"sam_lifelike/{k}": v for k, v in L.xz_copies(text).items()})
    return out


def zstd_files():
    return {os.path.relpath(p, GOLDEN): open(p, "rb").read() for d in ("zstd", "zstd_frames", "zstd_lifelike")
            for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.zst")))}


def decoded(codec: str):
    """[(name, bytes, text, Counter)] of every input of a codec."""
    files, decode = (xz_files(), lzma_paths.decode) if codec == "xz" else (zstd_files(), zstd_paths.decode)
    return [(name, blob) + decode(blob) for name, blob in files.items()]


def census(rows_xz=None, rows_zstd=None) -> dict:
    """What committed_inputs.json holds: per codec the files, the summed path counts and the paths at count 0."""
    out = {}
    for codec, rows, mod in (("xz", rows_xz, lzma_paths), ("zstd", rows_zstd, zstd_paths)):
        rows = rows if rows is not None else decoded(codec)
        total = Counter()
        for _, _, _, c in rows:
            total += c
        out[codec] = {"files": len(rows), "text_bytes": sum(len(t) for _, _, t, _ in rows), "paths": dict(sorted(total.items())),
                      "never_reached": [p for p in mod.all_paths() if not total[p]]}
    return out
