"""CPU tests of the lzip format code (slimm_amd/csrc/lzip_member.h, lzip_walk.h, host/lzip.cpp, and xz_stream.h's lzma_run with
the marked end) through the stand-alone program tests/native/san_lzip.cpp, built here under AddressSanitizer and UBSan: the
C++ member finder against the Python walker of tests/sam_lzip.py on every committed and written file, whole, a byte a peek,
and at every cut of a short file; the host decoder's text against Python's raw LZMA decoder member by member; every refused
directed input (tests/lzip_directed.py) refused in its own words, and by the reference too; the backward index against the
forward walk; the committed fixtures against their texts.  No GPU is touched."""
import os
import subprocess
import tempfile

import pytest

from tests import lzip_directed as LD
from tests import sam_lzip as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def san_lzip(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_lzip")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(NATIVE, "san_lzip.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "lzip.cpp"), "-o", exe], check=True)
    return exe


_made = {}


def made():
    """The texts, the committed files, the written copies and the 50-record text's directed inputs: made once."""
    if not _made:
        with tempfile.TemporaryDirectory() as d:
            texts = {(g, n): Z.case_text(d, g, n) for g, n in ((True, 50), (True, 3_000), (False, 3_000), (True, 1_000), (False, 1_000))}
        t = texts[(True, 50)]
        skip = Z.header_len(t)
        good, bad = LD.INPUTS(t[:skip], t[skip:])
        files = {}
        for kind, (n, name, tags) in Z.GOLDEN_KINDS.items():
            for tag in tags:
                files[name.format(tag)] = (Z.golden(name.format(tag)), texts[(tag == "grouped", n)])
        for kind, blob in Z.written_copies(texts[(True, 1_000)]).items():
            files["written_" + kind] = (blob, texts[(True, 1_000)])
        for name, (blob, text, _) in good.items():
            files["directed_" + name] = (blob, text)
        _made.update(texts=texts, files=files, good=good, bad=bad)
    return _made


def run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return r


def lines_of(blob):
    return [f"member {m['at']} {m['size']} {m['dict_size']} {m['data_size']} {m['crc']:08x}" for m in Z.walk(blob)]


def test_the_committed_files_hold_their_texts_and_are_what_their_names_say():
    m = made()
    for name, (blob, text) in m["files"].items():
        assert Z.decode(blob) == text, name
    c = {name: Z.census(blob) for name, (blob, _) in m["files"].items()}
    assert c["config1_grouped_m17.sam.lz"]["members"] == c["config1_any_m17.sam.lz"]["members"] == 17
    assert c["short_grouped_one.sam.lz"]["members"] == 1
    d4k = c["short_grouped_d4k.sam.lz"]
    assert d4k["max_dict"] == 4096 and d4k["members"] == -(-d4k["text_bytes"] // (20 << 10))
    assert c["short_any_empty_between.sam.lz"]["empty_members"] == 1 and c["short_any_empty_between.sam.lz"]["members"] == 4
    xz_largest = max(os.path.getsize(os.path.join(os.path.dirname(Z.GOLDEN), "xz", f)) for f in os.listdir(os.path.join(os.path.dirname(Z.GOLDEN), "xz")))
    assert all(os.path.getsize(os.path.join(Z.GOLDEN, f)) <= xz_largest for f in os.listdir(Z.GOLDEN))


def test_the_walker_is_the_python_walker_whole_and_a_byte_a_peek(san_lzip, tmp_path):
    """... and a byte a peek looks at every byte once: the search's cursor (no more than the file's bytes in all)."""
    for name, (blob, _) in made()["files"].items():
        p = str(tmp_path / "x.lz")
        open(p, "wb").write(blob)
        want = lines_of(blob)
        assert run(san_lzip, "--walk", p).stdout.split("\n")[:-1] == want, name
        if len(blob) > 12_000:
            continue
        for step in ("1", "7"):
            got = run(san_lzip, "--feed", step, p).stdout.split("\n")[:-1]
            assert got[:-1] == want, (name, step)
            _, peeks, _, searched = got[-1].split()
            assert int(searched) <= len(blob) and int(peeks) <= len(blob) + 2 * len(want) + 2, (name, got[-1])


def test_the_walker_at_every_cut_of_a_short_file(san_lzip, tmp_path):
    """The three-member directed file cut at every length: the members that are whole, then `truncated` -- or, where a cut
    leaves whole members and nothing else, the end."""
    blob = made()["good"]["empty_member_between"][0]
    ms = Z.walk(blob)
    ends = [m["at"] + m["size"] for m in ms]
    assert len(blob) < 2_000
    for n in range(len(blob) + 1):
        p = str(tmp_path / "x.lz")
        open(p, "wb").write(blob[:n])
        got = run(san_lzip, "--walk", p).stdout.split("\n")[:-1]
        whole = [e for e in ends if e <= n]
        assert got[:len(whole)] == lines_of(blob)[:len(whole)], n
        rest = got[len(whole):]
        if n in ends:
            assert rest == [], (n, rest)
        elif n == 0:
            assert rest == ["error member at byte 0: bytes that start no lzip member"] or "truncated" in rest[0], rest
        else:
            assert rest == [f"error member at byte {whole[-1] if whole else 0}: truncated"], (n, rest)


def test_the_host_decoder_gives_the_reference_decoders_text_member_by_member(san_lzip, tmp_path):
    for name, (blob, text) in made()["files"].items():
        p, out = str(tmp_path / "x.lz"), str(tmp_path / "m")
        open(p, "wb").write(blob)
        r = run(san_lzip, p)
        fields = r.stdout.strip().split("\t")
        assert fields[1] == "ok" and int(fields[2]) == len(text), (name, r.stdout)
        ms = Z.walk(blob)
        members, empty, match_bytes, max_dist, max_dict = map(int, fields[4].split())
        c = Z.census(blob)
        assert (members, empty, max_dict) == (c["members"], c["empty_members"], c["max_dict"]) and max_dist <= max(m["data_size"] for m in ms), (name, fields)
        assert run(san_lzip, "--members", out, p).returncode == 0
        for k, m in enumerate(ms):
            assert open(f"{out}.{k}", "rb").read() == Z.decode_member(blob, m), (name, k)


@pytest.mark.parametrize("name", sorted(LD.REFUSED))
def test_a_refused_directed_input_is_refused_in_its_own_words_and_by_the_reference(san_lzip, tmp_path, name):
    """(liblzma's raw decoder ends at a marker of any length -- lengths other than 2 are lzip's own rule -- so of the two
    marker-length inputs the reference says nothing: LD.REFERENCE_TAKES, held here to be exactly those.)"""
    blob = made()["bad"][name]
    p = str(tmp_path / "x.lz")
    open(p, "wb").write(blob)
    r = run(san_lzip, p)
    assert r.stdout.strip().split("\t")[1:] == ["error", LD.REFUSED[name]], r.stdout
    assert Z.refused_by_reference(blob) == (name not in LD.REFERENCE_TAKES), name


@pytest.mark.parametrize("name", Z.DAMAGE)
def test_damage_is_refused_in_words_and_by_the_reference(san_lzip, tmp_path, name):
    good, cases = Z.damaged(made()["texts"][(True, 1_000)])
    blob, words = cases[name]
    p = str(tmp_path / "x.lz")
    open(p, "wb").write(blob)
    r = run(san_lzip, p)
    assert r.stdout.strip().split("\t")[1] == "error" and words in r.stdout, r.stdout
    assert Z.refused_by_reference(blob), name
    assert sorted(cases) == sorted(Z.DAMAGE)


def test_the_backward_index_is_the_forward_walk(san_lzip, tmp_path):
    """... and does not close on byte 0 for a file with trailing data, a truncated one, or one with a damaged member_size."""
    m = made()
    for name, (blob, _) in m["files"].items():
        p = str(tmp_path / "x.lz")
        open(p, "wb").write(blob)
        want = [f"member {w['at']} {w['size']} {w['data_size']}" for w in Z.walk(blob)]
        assert run(san_lzip, "--index", p).stdout.split("\n")[:-1] == want, name
        assert [f"member {a} {s} {d}" for a, s, d in Z.walk_back(blob)] == want, name
    good, cases = Z.damaged(m["texts"][(True, 1_000)])
    for name in ("trailing_data", "inside_the_last_trailer", "inside_the_stream", "version_0", "not_lzip"):
        p = str(tmp_path / "x.lz")
        open(p, "wb").write(cases[name][0])
        assert run(san_lzip, "--index", p).stdout == "error\n" and Z.walk_back(cases[name][0]) is None, name
