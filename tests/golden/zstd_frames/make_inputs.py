"""Makes the multi-frame inputs of the split tests (run from the repository's root with libzstd on the machine:
`python tests/golden/zstd_frames/make_inputs.py`): the 3 000-record config1 text of tests/sam_zst.py, grouped and shuffled,
cut into 7 pieces anywhere -- so inside lines -- each piece one frame of libzstd's at level 3, and again at level 19, with
the 12-byte skippable frame in front of every frame by which pzstd states the frame's compressed size.
tests/test_split_zstd_ranges.py makes the texts again from their seeds and checks the files."""
import os
import struct
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_zst as Z  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PIECES = 7


def frames_of(text: bytes, level: int) -> bytes:
    out = []
    for piece in Z.cut_lines(text, PIECES):
        frame = Z.compress(piece, level)
        out.append(struct.pack("<III", 0x184D2A50, 4, len(frame)) + frame)
    return b"".join(out)


def main():
    with tempfile.TemporaryDirectory() as d:
        for grouped in (True, False):
            tag = "grouped" if grouped else "any"
            text = Z.case_text(d, grouped, 3_000)
            for level in (3, 19):
                name = f"config1_{tag}_frames_l{level}.sam.zst"
                blob = frames_of(text, level)
                open(os.path.join(HERE, name), "wb").write(blob)
                print(name, len(text), len(blob), {k: v for k, v in Z.census(blob).items() if v})


if __name__ == "__main__":
    main()
