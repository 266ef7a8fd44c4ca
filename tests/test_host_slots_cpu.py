"""The staging-slot grouping rules (csrc/host_slots.h) on the CPU, no GPU and no library: tests/cpp/host_slots_test.cc
runs the header that crc32c_host.cpp calls with tiny limits (slot_bytes / max_blocks = 64 / 4, 48 / 3, 16 / 1) over every
short sequence of a small alphabet and over seeded random sequences, checks that groups and long blocks partition the
call, stay within both limits, are maximal, and that the plan, executed against a byte buffer through a fake slot, gives
the CRC-32C of the caller's own bytes.  Each `--rule=<mutant>` swaps in a deliberately wrong rule and must fail: the
program can tell a wrong `<` for `<=`, a wrong base of the relative offsets or a missing round-up from the shipped rule.
The mutants run only in this CPU program, never in the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

MUTANTS = {
    "rel_first": "span",      # staged offsets against the first block's off, not the group's lo
    "cap_plus1": "",          # a block cap of max_blocks + 1
    "no_round": "gather",     # packing without the 16-B round-up
    "fit_no_round": "gather",  # the fit test ignores the round-up
    "long_ge": "",            # len >= slot_bytes treated as long
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_slots") / "host_slots_test"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "kv-separate_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "host_slots_test.cc"), "-o", str(out)])
    return str(out)


def test_shipped_rules_hold_every_property(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout and "shipped rule:" in r.stdout and " 0 failed" in r.stdout


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_wrong_rule_fails(exe, mutant):
    r = subprocess.run([exe, "--rule=" + mutant], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FAIL" in r.stdout and "PASS" not in r.stdout
    assert f"{mutant} rule:" in r.stdout
    first = next(l for l in r.stdout.splitlines() if l.startswith("FAILED "))
    assert first.startswith("FAILED " + MUTANTS[mutant]), first  # caught in the form the mutant breaks


def test_unknown_rule_is_refused(exe):
    # a misspelt mutant must not run the shipped rule and "pass"
    assert subprocess.run([exe, "--rule=nonsense"], capture_output=True, timeout=60).returncode == 2


def test_library_takes_its_grouping_from_the_header():
    """crc32c_host.cpp keeps no grouping arithmetic of its own: the two limits and the three rules live in
    host_slots.h, the file the program above includes."""
    src = open(os.path.join(ROOT, "kv-separate_amd", "csrc", "crc32c_host.cpp")).read()
    assert '#include "host_slots.h"' in src
    for call in ("slots::span_group(", "slots::span_at(", "slots::gather_group(", "slots::segment_count(",
                 "slots::segment(", "slots::is_long("):
        assert call in src, call
    for own in ("kSlotBytes =", "kSlotBlocks =", "1ull << 16", "& ~uint64_t(15)", "> s.bytes", ">= s.bytes"):
        assert own not in src, own
