"""CPU tests of the lifelike inputs (tests/sam_lifelike.py): the text is the same on every machine -- one sha256 is pinned --
and holds what it promises; tests/bam_io.bam_record_bytes writes what it wrote before where the lifelike option is off; the
committed zstd files of tests/golden/zstd_lifelike are the texts of their seed and hold what the device tests ask of them.
No GPU is touched."""
import hashlib
import os
import struct
import subprocess

import pytest

from tests import sam_lifelike as L
from tests import sam_zst as Z
from tests.bam_io import bam_record_bytes
from tests.sam_gz import header_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = {False: "36f2572ed38960b5", True: "afa8a7a63d8e0813"}   # (hi_bytes: the first 16 hex digits, config1, seed 31, 1 000 records, grouped)


def test_the_text_is_the_same_everywhere_and_looks_like_a_sam_file():
    w = Z.case_workload(True, 1_000)
    for hi in (False, True):
        text = L.lifelike_text(w, 31, hi_bytes=hi)
        assert hashlib.sha256(text).hexdigest()[:16] == PINNED[hi]
        assert text == L.lifelike_text(w, 31, hi_bytes=hi) and text != L.lifelike_text(w, 32, hi_bytes=hi)
        lines = text[header_len(text):].split(b"\n")
        assert lines.pop() == b"" and len(lines) == len(w.records)
        lens, quals, n_bases = [], bytearray(), 0
        for i, line in enumerate(lines):
            f = line.split(b"\t")
            assert 13 <= len(f) <= 15 + hi, line
            assert f[0].decode() == w.records.qname[i] and int(f[1]) == int(w.records.flag[i]) and int(f[3]) == int(w.records.begin_pos[i]) + 1
            if f[9] == b"*":
                assert f[10] == b"*" and f[5] == b"*"
                lens.append(0)
                continue
            assert len(f[9]) == len(f[10]) and set(f[9]) <= set(b"ACGTN")
            # the CIGAR's query-consuming operations add up to the sequence
            ops, n = [], b""
            for c in f[5]:
                if 48 <= c <= 57:
                    n += bytes([c])
                else:
                    ops.append((int(n), chr(c)))
                    n = b""
            assert sum(k for k, op in ops if op in "MIS") == len(f[9]), line
            lens.append(len(f[9]))
            n_bases += f[9].count(b"N")
            quals += f[10]
            assert f[11].startswith(b"NM:i:") and f[12].startswith(b"MD:Z:")
            if hi:
                assert f[-1].startswith(b"XB:Z:") and len(f[-1]) <= 45 and all(c >= 128 for c in f[-1][5:])
        assert lens[3] == 1 and lens[7] == 2 and 1 <= lens.count(0) <= 40 and max(lens) > 290
        assert min(quals) == 33 and max(quals) >= 110 and 66 <= sorted(quals)[len(quals) // 2] <= 70
        assert 0.005 < n_bases / sum(lens) < 0.015
        assert (max(text) >= 0x80) == hi


def test_bam_record_bytes_is_unchanged_where_the_option_is_off_and_lifelike_where_it_is_on():
    w = Z.case_workload(True, 1_000)
    assert hashlib.sha256(bam_record_bytes(w.records)).hexdigest()[:12] == "064724927868"
    assert hashlib.sha256(bam_record_bytes(w.records, irregular_seed=7)).hexdigest()[:12] == "59b6d7213217"
    data = bam_record_bytes(w.records, lifelike_seed=31)
    assert data == bam_record_bytes(w.records, lifelike_seed=31) != bam_record_bytes(w.records, lifelike_seed=32)
    p, lens, quals = 0, [], bytearray()
    for i in range(len(w.records)):
        size, ref, pos, l_name, mapq, _, n_op, flag, l_seq = struct.unpack_from("<iiiBBHHHI", data, p)
        assert (ref, pos, flag) == (int(w.records.ref_id[i]), int(w.records.begin_pos[i]), int(w.records.flag[i]))
        at = p + 36 + l_name
        cigar = struct.unpack_from(f"<{n_op}I", data, at)
        assert sum(c >> 4 for c in cigar if (c & 15) in (0, 1, 4)) == l_seq
        at += 4 * n_op + (l_seq + 1) // 2
        quals += data[at:at + l_seq]
        assert data[at + l_seq:p + 4 + size][:3] == b"NMC"
        lens.append(l_seq)
        p += 4 + size
    assert p == len(data) and lens[3] == 1 and lens[7] == 2 and 0 in lens and max(lens) > 290
    assert min(quals) == 0 and max(quals) == 93
    blob, skip, body = L.lifelike_bam(w, 31)
    assert body == data and skip > 0


@pytest.fixture(scope="module")
def san_zstd(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_zstd")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_zstd.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "zstd.cpp"), "-o", exe],
                   check=True)
    return exe


def test_the_committed_zstd_inputs_are_the_texts_of_their_seed(san_zstd, tmp_path):
    """Levels 1 and 19, windowLog 10, and a frame without checksum and content size, of the 300-record text: each the text of
    its seed by the host decoder (and by ZSTD_decompress where the machine has libzstd), with a Huffman tree, FSE-described
    tables and more than 1 000 sequences' worth of blocks, and no larger than the largest file tests/golden held before."""
    golden = os.path.join(ROOT, "tests", "golden")
    largest = max(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(golden) if "zstd_lifelike" not in d for f in fs)
    for kind, (name, hi, level, window_log, stated) in L.ZSTD_KINDS.items():
        blob, text = L.zstd_golden(kind), L.zstd_text(kind)
        assert len(blob) <= largest, (name, len(blob), largest)
        assert (max(text) >= 0x80) == hi and 1.2 < len(text) / len(blob) < 3.5, name
        p, out = str(tmp_path / name), str(tmp_path / (name + ".out"))
        open(p, "wb").write(blob)
        r = subprocess.run([san_zstd, "--out", out, p], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (name, r.stderr[-2000:])
        assert open(out, "rb").read() == text, name
        if Z.LIB is not None:
            assert Z.decompress(blob, len(text) + 1) == text, name
        (frame,), c = Z.walk(blob), Z.census(blob)
        assert c["frames"] == 1 and c["lit_huffman"] >= 1 and c["fse_tables"] >= 3 and c["raw"] == c["rle"] == 0, (name, c)
        assert (frame["checksum_at"] is not None) == stated and (frame["content_size"] is not None) == stated, name
        assert (frame["window"] == 1024) == (window_log == 10), (name, frame["window"])
        assert sum(b["n_seq"] for b in frame["blocks"]) > 1_000, name
        assert c["compressed"] >= (100 if window_log == 10 else 1), (name, c)
