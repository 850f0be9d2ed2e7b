"""Makes the compressor-made inputs of the zstd tests (run from the repository's root with libzstd on the machine:
`python tests/golden/zstd/make_inputs.py`): the 3 000-record config1 text of the gzip tests at levels 3 and 19, and a
shorter text at windowLog 10.  tests/test_zstd_frame.py makes the texts again from their seeds and checks the files."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_zst as Z  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    with tempfile.TemporaryDirectory() as d:
        for grouped in (True, False):
            tag = "grouped" if grouped else "any"
            text = Z.case_text(d, grouped, 3_000)
            short = Z.case_text(d, grouped, 400)
            for name, blob in ((f"config1_{tag}_l3.sam.zst", Z.compress(text, 3)), (f"config1_{tag}_l19.sam.zst", Z.compress(text, 19)),
                               (f"short_{tag}_wlog10.sam.zst", Z.compress(short, 3, window_log=10))):
                open(os.path.join(HERE, name), "wb").write(blob)
                print(name, len(blob), {k: v for k, v in Z.census(blob).items() if v})


if __name__ == "__main__":
    main()
