"""The record filter's options of the `slimm` command: --help names them, and a value out of range is a usage error with
status 1 given before the database is opened (the database named here does not exist).  No GPU is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True)


def test_help_names_the_options():
    r = run(["--help"])
    assert r.returncode == 0
    for opt in ("-q", "--min-mapq", "--require-flags", "--exclude-flags", "--min-aligned", "--min-identity"):
        assert opt in r.stderr, opt


@pytest.mark.parametrize("args,word", [
    (["-q", "-1"], "min-mapq"), (["-q", "256"], "min-mapq"), (["--min-mapq", "ten"], "min-mapq"), (["-q", "0x10"], "min-mapq"),
    (["--require-flags", "0x10000"], "require-flags"), (["--require-flags", "65536"], "require-flags"), (["--require-flags", "-2"], "require-flags"),
    (["--exclude-flags", "0xZZ"], "exclude-flags"), (["--exclude-flags", ""], "exclude-flags"), (["--exclude-flags", "1e3"], "exclude-flags"),
    (["--min-aligned", "-5"], "min-aligned"), (["--min-aligned", "4294967296"], "min-aligned"), (["--min-aligned", "50bp"], "min-aligned"),
    (["--min-identity", "1.01"], "min-identity"), (["--min-identity", "-0.1"], "min-identity"), (["--min-identity", "95%"], "min-identity"),
    (["--min-identity", "nan"], "min-identity"), (["--min-identity", ""], "min-identity"),
])
def test_values_out_of_range_are_usage_errors(tmp_path, args, word):
    missing = str(tmp_path / "no_such.sldb")
    r = run(args + [missing, str(tmp_path / "no_such.bam")])
    assert r.returncode == 1
    assert word in r.stderr
    assert "no_such" not in r.stderr   # (neither the database nor the input was looked at)


@pytest.mark.parametrize("args", [["-q", "255"], ["--require-flags", "0xffff", "--exclude-flags", "65535"], ["--min-aligned", "0"],
                                  ["--min-identity", "1"], ["--min-identity", "0.0"]])
def test_values_in_range_get_as_far_as_the_input(tmp_path, args):
    r = run(args + [str(tmp_path / "no_such.sldb"), str(tmp_path / "no_such.bam")])
    assert r.returncode == 1 and "no_such" in r.stderr
