"""`slimm --file-per-device`: what the command refuses before it loads a database or touches a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")


def run(args):
    # (neither the database nor the input exists: a run that got as far as either would say so, not this)
    return subprocess.run([CLI] + args + ["no_such.sldb", "no_such_directory"], capture_output=True, text=True)


def test_file_per_device_with_split_input_is_a_usage_error():
    r = run(["-d", "--file-per-device", "--devices", "0,0", "--split-input"])
    assert r.returncode == 1
    assert "--file-per-device and --split-input exclude each other" in r.stderr
    assert "no_such" not in r.stderr
    r = run(["-d", "--split-input", "--devices", "0,0", "--file-per-device"])   # (in any order on the line)
    assert r.returncode == 1 and "--file-per-device and --split-input exclude each other" in r.stderr


def test_file_per_device_without_devices_is_a_usage_error():
    for extra in ([], ["--device", "0"]):
        r = run(["-d", "--file-per-device"] + extra)
        assert r.returncode == 1
        assert "--file-per-device needs --devices" in r.stderr
        assert "no_such" not in r.stderr


def test_usage_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--file-per-device" in r.stderr
