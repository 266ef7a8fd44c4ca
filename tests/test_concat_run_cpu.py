"""The run arithmetic of crc32c_concat_kernel (csrc/concat_run.h) on the CPU, no GPU and no library:
tests/cpp/concat_run_test.cc emulates the kernel's launch lane by lane with the header the kernel itself includes --
the clamp of first[], the short / long split, the passes, the per-lane chunks, the ordered lane tree and the affine
operator -- over every first[] of a small alphabet for count <= 4, nseg <= 5 (decreasing values and values above nseg
included), over the same with runs long enough for the wavefront path, and over seeded random batches with runs of up to
three passes.  Every case must give the plain serial fold and touch no index outside the arrays.  Each
`--rule=<mutant>` swaps in a deliberately wrong rule and must fail.  The mutants run only in this CPU program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

MUTANTS = {
    "swap": "differs from the serial fold",        # the operator with its operands swapped
    "no_clamp": "a segment index >= nseg was read",  # first[] used as it comes
    "chunk_floor": "differs from the serial fold",  # floor(n / 64) segments per lane: the last ones are dropped
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("concat_run") / "concat_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "concat_run_test.cc"), "-o", str(out)])
    return str(out)


def test_shipped_rules_give_the_serial_fold_inside_the_arrays(exe):
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
    assert MUTANTS[mutant] in first, first  # caught for the reason the mutant is wrong


def test_unknown_rule_is_refused(exe):
    # a misspelt mutant must not run the shipped rule and "pass"
    assert subprocess.run([exe, "--rule=nonsense"], capture_output=True, timeout=60).returncode == 2


def test_kernel_and_host_fold_take_their_runs_from_the_header():
    """Neither the kernel nor the host fold of the gather form keeps index arithmetic of its own: the clamp, the split,
    the passes, the chunks and the tree come from concat_run.h, the file the program above includes."""
    kernel = open(os.path.join(CSRC, "crc32c_concat.inc")).read()
    for call in ("concat::clamp_run(", "concat::is_short(", "concat::pass_end(", "concat::lane_chunk(",
                 "concat::lane_range(", "concat::compose(", "concat::tree_joins(", "concat::identity("):
        assert call in kernel, call
    host = open(os.path.join(CSRC, "crc32c_host.cpp")).read()
    assert '#include "concat_run.h"' in host and "concat::clamp_run(" in host
    header = open(os.path.join(CSRC, "concat_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
