"""CPU test of the BGZF block header walk (slimm_amd/csrc/bgzf_block.h: what the command's reader and the library's
descriptor walk both parse a block with), through the stand-alone program tests/native/san_bgzf_block.cpp built under
AddressSanitizer and UBSan.  The program hands every block over in a heap buffer of exactly the bytes it speaks of, so one read
too far is a sanitizer report; this file asserts on the cases' lines and on an empty report.  No GPU is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("canonical", "canonical/every-prefix", "subfield-in-front", "subfield-behind", "subfields-on-both-sides",
         "subfields-on-both-sides/every-prefix", "bc-last", "empty-payload", "bc-of-three-bytes", "bc-of-no-bytes", "other-subfields-only",
         "xlen-0", "slen-past-xlen", "slen-past-xlen-alone", "bc-cut-by-xlen", "bsize-below-header-and-trailer", "bsize-0",
         "bsize-of-header-and-trailer", "bsize-beyond-the-bytes", "isize-65536", "isize-65537", "isize-2^32-1",
         *(f"wrong-byte-{k}{tail}" for k in range(4) for tail in ("", "/12-bytes")), "flg-with-more-bits",
         "eof-block-is-28-bytes", "eof-block", "eof-block-behind-subfields", "eof-near-miss-crc", "eof-near-miss-payload",
         "eof-near-miss-isize", "eof-near-miss-three-bytes")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_bgzf_block")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_bgzf_block.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_no_byte_beyond_the_block_is_read(run):
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr.strip() == "", run.stderr[-2000:]


def test_every_case_answers_as_the_format_says(run):
    lines = dict(ln.split("\t", 1) for ln in run.stdout.splitlines())
    assert run.returncode == 0 and lines.pop("failed") == "0", run.stdout
    assert {k: v for k, v in lines.items() if v != "ok"} == {}
    assert sorted(lines) == sorted(CASES)
