"""Writes committed_inputs.json, the census of tests/codec_census.py: which paths of the LZMA and zstd entropy decoders the
committed xz and zstd inputs reach, and which they never do.  Run from the repository's root:
    python tests/golden/codec_paths/make_census.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import codec_census  # noqa: E402

if __name__ == "__main__":
    with open(codec_census.JSON, "w") as f:
        json.dump(codec_census.census(), f, indent=1, sort_keys=True)
        f.write("\n")
