"""Makes the committed inputs of the lzip tests (run from the repository's root: `python tests/golden/lzip/make_inputs.py`).
The members are written with Python's `lzma` (tests/sam_lzip.py: member) -- liblzma's output differs between versions, so the
files are committed, not made again by the tests:
  config1_{grouped,any}_m17.sam.lz    the 3 000-record config1 text in 17 members cut at any byte, as `plzip` cuts: the
                                      command's default takes the device from 16 members on
  short_grouped_one.sam.lz            the 1 000-record text as one member
  short_grouped_d4k.sam.lz            ... with a 4 KiB dictionary in members of 20 KiB of text: the window slides
  short_any_empty_between.sam.lz      ... in three members with an empty one among them
tests/test_lzip_member.py makes the texts again from their seeds and checks the files."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_lzip as Z  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def made(d) -> dict:
    out = {}
    for grouped in (True, False):
        tag = "grouped" if grouped else "any"
        text = Z.case_text(d, grouped, 3_000)
        out[f"config1_{tag}_m17.sam.lz"] = (Z.members(text, -(-len(text) // 17)), text)
    short = Z.case_text(d, True, 1_000)
    out["short_grouped_one.sam.lz"] = (Z.member(short, 1 << 20), short)
    out["short_grouped_d4k.sam.lz"] = (Z.members(short, 20 << 10, 4096), short)
    short = Z.case_text(d, False, 1_000)
    a, b, c = Z.cut_lines(short, 3)
    out["short_any_empty_between.sam.lz"] = (Z.member(a) + Z.member(b"") + Z.member(b) + Z.member(c), short)
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        for name, (blob, text) in made(d).items():
            assert Z.decode(blob) == text
            open(os.path.join(HERE, name), "wb").write(blob)
            print(name, len(blob), Z.census(blob))


if __name__ == "__main__":
    main()
