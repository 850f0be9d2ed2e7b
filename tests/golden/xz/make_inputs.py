"""Makes the compressor-made inputs of the xz tests (run from the repository's root with `xz` 5.2.5 on the machine:
`python tests/golden/xz/make_inputs.py`): the 3 000-record config1 text of the gzip tests in many blocks, with and without
sizes in the block headers; a 15 000-record text in one block, long enough for a second LZMA chunk; a 1 000-record text under
other presets, literal settings and check kinds, behind the x86 filter (to be refused), and in three pieces compressed one by
one (the blocks that tests/sam_xz.py wraps again).  tests/test_xz_stream.py makes the texts again from their seeds and
checks the files."""
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_xz as X  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ARGS = {
    "mt": ["-6", "-T2", "--block-size=32KiB"], "blocks": ["-6", "--block-size=32KiB"], "one": ["-6"], "l0": ["-0"], "l9e": ["-9e"],
    "lc0lp2": ["--lzma2=preset=6,lc=0,lp=2,pb=0", "--check=crc32"], "lc4": ["--lzma2=preset=6,lc=4,lp=0,pb=2"], "none": ["--check=none"],
    "sha256": ["--check=sha256"],
}
PART_ARGS = (["-6"], ["-0"], ["--lzma2=preset=6,lc=1,lp=1,pb=1"])


def xz(args, text: bytes) -> bytes:
    return subprocess.run(["xz", "-c"] + args, input=text, capture_output=True, check=True).stdout


def main():
    with tempfile.TemporaryDirectory() as d:
        for grouped in (True, False):
            tag = "grouped" if grouped else "any"
            made = {name.format(tag): xz(ARGS[kind], X.case_text(d, grouped, n)) for kind, (n, name) in X.GOLDEN_KINDS.items()}
            short = X.case_text(d, grouped, X.PARTS[0])
            for i, part in enumerate(X.cut_lines(short, 3)):
                made[X.PARTS[1].format(tag, i)] = xz(PART_ARGS[i], part)
            for name, blob in made.items():
                open(os.path.join(HERE, name), "wb").write(blob)
                print(name, len(blob), {k: v for k, v in X.census(blob).items() if v})
            name = X.REFUSED_KIND[1].format(tag)
            open(os.path.join(HERE, name), "wb").write(xz(["--x86", "--lzma2"], short))
            print(name, os.path.getsize(os.path.join(HERE, name)))


if __name__ == "__main__":
    main()
