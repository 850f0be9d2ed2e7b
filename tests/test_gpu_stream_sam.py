"""The streamed codecs' shared path on a real MI355X (windows.hip: push_stream, check_push, open_file; the file state every
codec keeps -- windows.h: File::Stream): what no single-codec test pins for all three.  slimm_push_bzip2_sam_bytes,
_gzip_sam_bytes and _zstd_sam_bytes against slimm_push_sam_bytes on the same text.  The inputs: tests/sam_bz2.py,
tests/sam_deflate.py, tests/sam_zst.py."""
import ctypes as C
import random

import numpy as np
import pytest

from slimm_amd.profiler import Slimm
from tests import sam_bz2 as B
from tests import sam_deflate as D
from tests import sam_zst as Z
from tests.test_gpu_compressed_sam import integers, profile_of

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
CODECS = ["bzip2", "gzip", "zstd"]
N_RECORDS = 300
ROUND_TEXT = 4096          # zstd_round_text below; the other codecs' rounds hold what a push of a few hundred bytes completes
HEADER = 6 * ROUND_TEXT    # the long header: several rounds' text
# rounds as small as the pushes: every push is decoded as far as it goes, and the rest waits for the next one
FORCE = {"bzip2": "bzip2_round=1", "gzip": "gzip_chunk=2048,gzip_round=1", "zstd": "zstd_round=1,zstd_round_text=4096"}


def compressed(codec, text):
    """`text` in blocks far smaller than its header: bzip2 streams of 3 000 bytes (cut anywhere: one holds the header's end
    and the first lines; an empty one among them), a gzip member of some hundred small dynamic blocks, a zstd frame of raw
    blocks of 1 000 bytes with a content checksum."""
    if codec == "bzip2":
        return B.streams(text, chunk=3_000, levels=(1, 9))
    if codec == "gzip":
        return D.copy_of(text, "mem1")
    return Z.raw_frame(text, step=1_000)


def push(s, codec, blob, **kw):
    return getattr(s, f"push_{codec}_sam_bytes")(blob, **kw)


def cuts_of(n, seed):   # pieces of a few hundred bytes
    rng, p, out = random.Random(seed), 0, []
    while True:
        p += rng.randint(200, 700)
        if p >= n:
            return out
        out.append(p)


_shared = {}


def case(tmp_path, long_header):
    """The 300-record text -- with its own header, or with comment lines added to it up to HEADER bytes --, the header's
    length and the profile of the plain text: made once."""
    if long_header not in _shared:
        w = Z.case_workload(True, N_RECORDS)
        text = Z.case_text(tmp_path, True, N_RECORDS)
        skip = Z.header_len(text)
        if long_header:
            rng, pad = random.Random(5), b""
            while skip + len(pad) < HEADER:
                pad += b"@CO\t" + ("%064x" % rng.getrandbits(256)).encode() + b"\n"
            text = text[:skip] + pad + text[skip:]
            skip += len(pad)
        s, want = profile_of(w, True, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[long_header] = (w, text, skip, want)
    return _shared[long_header]


@pytest.mark.parametrize("codec", CODECS)
def test_a_header_longer_than_several_rounds_text(tmp_path, monkeypatch, codec):
    """`skip` spans rounds: what is left of it is carried over more than one emit, the first rounds are header only and
    make no window, and one round holds the header's end and the first lines.  Closed with the last piece, or with an
    empty push behind it."""
    w, text, skip, want = case(tmp_path, True)
    assert skip >= HEADER and Z.header_len(text) == skip
    blob = compressed(codec, text)
    monkeypatch.setenv("SLIMM_FORCE", FORCE[codec])
    for empty_last in (False, True):
        s, got = profile_of(w, True, lambda s: push(s, codec, blob, skip=skip, cuts=cuts_of(len(blob), 3), empty_last=empty_last))
        assert got == want
        # (the counters that outlive the file say that every byte went through; zstd: a round holds at most four raw blocks
        # -- zstd_round_text --, so the header alone is six rounds or more.  The other codecs' rounds are as many as the
        # pushes that complete a block: about forty for these inputs under the host emulator, by SLIMM_TRACE=push)
        st = {"bzip2": dict, "gzip": s.gzip_stats, "zstd": s.zstd_stats}[codec]()
        if st:
            assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob), st
        if codec == "zstd":
            assert st["rounds"] * ROUND_TEXT >= len(text), st
        s.close()


def test_three_files_of_three_codecs_through_one_context(tmp_path, monkeypatch):
    """Nothing of one codec's file state survives slimm_reset into the next file, in any order of the codecs; and within a
    file a second codec is refused with the words the first one's mismatch has today."""
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    w, text, skip, want = case(tmp_path, False)
    blobs = {k: compressed(k, text) for k in CODECS}
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    for codec in CODECS + CODECS[::-1]:
        assert push(s, codec, blobs[codec], skip=skip, window=5_000) == len(w.records)
        s.get_profiles()
        assert integers(s) == want, codec
        s.reset()
    got = C.c_uint64()
    for a in CODECS:
        for b in CODECS:
            if a == b:
                continue
            one, two = (np.frombuffer(blobs[k], dtype=np.uint8).copy() for k in (a, b))
            rc = getattr(s.L, f"slimm_push_{a}_sam_bytes")(s.ctx, one.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got))
            assert rc == SLIMM_OK, (a, s.L.slimm_last_error(s.ctx).decode())
            rc = getattr(s.L, f"slimm_push_{b}_sam_bytes")(s.ctx, two.ctypes.data_as(C.c_void_p), 100, 0, 0, C.byref(got))
            assert rc == SLIMM_E_INVALID, (a, b)
            first = min(a, b, key=CODECS.index)   # (the checks come in the codecs' order: the first that sees a mismatch speaks)
            assert s.L.slimm_last_error(s.ctx).decode() == f"{first} SAM bytes and the other forms do not mix within a file", (a, b)
            s.reset()
    # ... and the context is as good as new
    assert push(s, "gzip", blobs["gzip"], skip=skip) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    s.close()


@pytest.mark.parametrize("codec", CODECS)
def test_a_push_behind_the_files_last_window_is_refused(tmp_path, monkeypatch, codec):
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    w, text, skip, want = case(tmp_path, False)
    blob = compressed(codec, text)
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert push(s, codec, blob, skip=skip) == len(w.records)
    got, buf = C.c_uint64(), np.frombuffer(blob, dtype=np.uint8).copy()
    for n, last in ((buf.size, 1), (100, 0), (0, 1)):
        rc = getattr(s.L, f"slimm_push_{codec}_sam_bytes")(s.ctx, buf.ctypes.data_as(C.c_void_p) if n else None, n, 0, last, C.byref(got))
        assert rc == SLIMM_E_INVALID and got.value == 0
        assert "reset first" in s.L.slimm_last_error(s.ctx).decode()
    s.reset()
    assert push(s, codec, blob, skip=skip, window=3_000) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    s.close()
