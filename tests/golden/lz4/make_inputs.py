"""Makes the compressor-made inputs of the lz4 tests (run from the repository's root with liblz4 on the machine:
`python tests/golden/lz4/make_inputs.py`): the 3 000-record config1 text of the gzip tests, grouped and in any order, as
independent blocks of 64 KiB, as linked blocks at level 9 with block checksums and a content size, and as the `lz4`
command's default frame (4 MiB blocks, a content checksum); and the 400-record text.  It also records, for every directed block of tests/sam_lz4.py, LZ4_decompress_safe's
verdict and the digest of what it gave (directed_verdicts.json).  tests/test_lz4_frame.py makes the texts again from their
seeds and checks the files."""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import sam_lz4 as L  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = {"b4": dict(block_id=4), "linked9": dict(block_id=4, linked=True, level=9, block_sums=True, content_size=True), "default": dict(block_id=7, checksum=True)}   # (default: the `lz4` command's, 4 MiB blocks and a content checksum)


def directed_blocks(header: bytes, records: bytes) -> dict:
    """{name: the block's bytes}: every compressed block of the directed inputs that stands alone (an independent frame's), the
    blocks of the directed errors, and the blocks only the decoders here take."""
    out = {}
    for name, (blob, _, _) in L.INPUTS(header, records, staging=False).items():
        for f in L.walk(blob):
            for k, b in enumerate(f["blocks"]):
                if not f["skippable"] and not f["linked"] and not b["stored"]:
                    out[f"{name}:{f['at']}:{k}"] = blob[b["at"] + 4:b["at"] + 4 + b["size"]]
    for name, (blob, _) in L.INVALID(header, records).items():
        f = L.walk(blob)[-1]
        b = f["blocks"][-2]
        out[f"invalid:{name}"] = blob[b["at"] + 4:b["at"] + 4 + b["size"]]
    for name, (body, _) in L.UNSAFE_BUT_TAKEN().items():
        out[f"taken:{name}"] = body
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        for grouped in (True, False):
            tag = "grouped" if grouped else "any"
            text = L.case_text(d, grouped, 3_000)
            for key, kw in SETTINGS.items():
                blob = L.compress(text, **kw)
                assert L.decode(blob) == text
                open(os.path.join(HERE, f"config1_{tag}_{key}.sam.lz4"), "wb").write(blob)
                print(f"config1_{tag}_{key}.sam.lz4", len(blob), {k: v for k, v in L.census(blob).items() if v})
        short = L.case_text(d, True, 400)
        blob = L.compress(short, block_id=4)
        open(os.path.join(HERE, "short_grouped_b4.sam.lz4"), "wb").write(blob)
        print("short_grouped_b4.sam.lz4", len(blob), {k: v for k, v in L.census(blob).items() if v})
        text = L.case_text(d, True, 50)
        skip = L.header_len(text)
        verdicts = {}
        for name, body in sorted(directed_blocks(text[:skip], text[skip:]).items()):
            got = L.decompress_safe(body, 1 << 17)
            verdicts[name] = {"block": L.digest(body), "accepted": got is not None, "text": L.digest(got) if got is not None else None}
        json.dump(verdicts, open(os.path.join(HERE, "directed_verdicts.json"), "w"), indent=1, sort_keys=True)
        print("directed_verdicts.json", len(verdicts), "blocks,", sum(v["accepted"] for v in verdicts.values()), "accepted")


if __name__ == "__main__":
    main()
