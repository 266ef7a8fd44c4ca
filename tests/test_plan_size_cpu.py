"""The plan sizing rules (csrc/plan_size.h) on the CPU, no GPU and no library: tests/cpp/plan_size_test.cc checks that
kvsep_crc32c_reserve(count, total) holds the plan of every smaller batch whatever piece size it picks, and of the SST
read check's len + 1 call, that piece_for is the rule its comment states, and that the reservation is exact.  The same
program run against the rule reserve used before (one piece size, the caller's own total) must fail at the piece-size
thresholds and on the SST form: the property is one that rule does not have."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan_size") / "plan_size_test"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "kv-separate_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plan_size_test.cc"), "-o", str(out)])
    return str(out)


def test_reservation_covers_every_smaller_batch(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout and " 0 failed" in r.stdout


def test_the_earlier_rule_fails_the_bound_property(exe):
    """reserve(n, want * P) planned P-byte pieces only, so a batch of want * P - 1 bytes (P / 2 pieces) did not fit:
    the deterministic grid must show exactly the thresholds (and +1, +2) for the batch form on 256 CUs, and the SST
    read check must fail too."""
    r = subprocess.run([exe, "--rule=parent"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout[-4000:]
    assert "FAIL" in r.stdout
    line = next(l for l in r.stdout.splitlines() if l.startswith("cus=256 piece=131072 auto:"))
    want = 2 * 256 * 8
    points = " ".join(str(want * p + d) for p in (32 << 10, 64 << 10, 128 << 10) for d in (0, 1, 2))
    assert f"at total = {points} (+" in line, line
    assert "SST read check at 22 of 22 grid totals" in line, line
    explicit = next(l for l in r.stdout.splitlines() if l.startswith("cus=256 piece=131072:"))
    assert "at total = (+0 random totals)" in explicit, explicit  # one P: only the SST form was short
