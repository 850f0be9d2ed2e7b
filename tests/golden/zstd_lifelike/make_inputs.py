"""Makes the compressor-made zstd inputs of the lifelike-text tests (run from the repository's root with libzstd on the
machine: `python tests/golden/zstd_lifelike/make_inputs.py`): the 300-record lifelike text (tests/sam_lifelike.py, config1,
seed 31, grouped) at levels 1 and 19, at windowLog 10, and without checksum and content size; two of them with bytes of
128 .. 255 in a tag.  tests/test_lifelike_inputs.py makes the texts again from their seed and checks the files."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_lifelike as L  # noqa: E402
from tests import sam_zst as Z  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    for kind, (name, hi, level, window_log, stated) in L.ZSTD_KINDS.items():
        blob = Z.compress(L.zstd_text(kind), level, window_log=window_log, content_size=stated, checksum=stated)
        open(os.path.join(HERE, name), "wb").write(blob)
        print(name, len(blob), {k: v for k, v in Z.census(blob).items() if v})


if __name__ == "__main__":
    main()
