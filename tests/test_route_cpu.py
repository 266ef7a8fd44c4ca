"""The routing rule (csrc/route.h) on the CPU, no GPU and no library: tests/cpp/route_test.cc carries the five routing
functions crc32c_device.hip had before the header, combined the way its launch and its two query entry points combined
them, and requires route::decide to equal them in every field on a grid of every threshold +- 1 and on 10^6 random
points.  The grid must reach every form and both schedules, and three deliberately wrong rules in decide's place must
each be caught."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("route") / "route_test"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "route_test.cc"), "-o", str(out)])
    return str(out)


def test_decide_equals_the_rule_it_replaced(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout and " 0 differ" in r.stdout and "UNREACHED" not in r.stdout
    # the grid shows itself: every form and both schedules were reached
    reached = dict((int(m.group(1)), int(m.group(2))) for m in re.finditer(r"form +(\d+) \S+ +(\d+) points", r.stdout))
    assert sorted(reached) == [0, 6, 9, 10, 11, 12, 20] and all(n > 0 for n in reached.values()), reached
    m = re.search(r"schedule static (\d+), guided (\d+)", r.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0
    m = re.search(r"(\d+) grid points, (\d+) random points", r.stdout)
    assert m and int(m.group(1)) > 10 ** 6 and int(m.group(2)) == 10 ** 6


@pytest.mark.parametrize("wrong", ["claim-bound", "ragged-order", "coop-hint"])
def test_a_wrong_rule_is_caught(exe, wrong):
    """The claim kernel's upper bound off by one, ragged tested after claim16, the coop hint left unclamped."""
    r = subprocess.run([exe, "--candidate=" + wrong], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout[-4000:]
    assert "FAIL" in r.stdout and "DIFF" in r.stdout and "UNREACHED" not in r.stdout


def test_the_device_file_routes_through_the_header_alone():
    """crc32c_device.hip holds no crossover of its own: none of the five functions, no form number as a bare literal in
    a case or a comparison, one narrow dispatch, and the only memset nodes are reset_vacc's."""
    src = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    for gone in ("ragged_batch", "claim16_route", "narrow_form", "use_narrow", "route_batch"):
        assert gone not in src, gone
    assert '#include "route.h"' in src and src.count("route::decide(") == 1
    assert not re.search(r"case (6|9|10|11|12|20):", src)
    assert not re.search(r"\b(nv|nf|form) == (6|9|10|11|12|20)\b", src)
    assert src.count("launch_narrow_v<true>") == 1 and src.count("launch_narrow_v<false>") == 1
    assert src.count("hipMemsetAsync(") == 2
    body = src[src.index("int reset_vacc("):]
    assert body[:body.index("\n}\n")].count("hipMemsetAsync(") == 2
    header = open(os.path.join(CSRC, "route.h")).read()
    assert "hip_runtime" not in header and "getenv" not in header
