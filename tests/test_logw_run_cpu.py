"""The rules of the log / MANIFEST write side (csrc/logw_run.h) on the CPU, no GPU.

tests/cpp/logw_run_test.cc is the control flow of the two kernels of csrc/crc32c_logframe.inc written lane by lane over
a memory model, with every decision taken from the header the kernels and kvsep_log_frame_layout include, against
log::Writer::AddRecord's loop restated serially: every output element written exactly once, nothing outside the stated
element counts, no dropped record's off used, no scratch word read that the call did not write, and three deliberately
wrong rules caught.  The program is built with AddressSanitizer and UBSan and run as it is."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("logw_run") / "logw_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "logw_run_test.cc"), "-o", str(out)])
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=900)


@needs_gxx
def test_the_kernels_reproduce_the_writers_loop(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "PASS" in run.stdout and " 0 failed" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    # 32,768 start offsets x 15 lengths, the sequences of up to three and the random rows
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 32768 * 15 + 7 * (15 + 225 + 3375)


@needs_gxx
def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"a trailer emitted after the last record", "a leftover of exactly 7 treated as a pad",
                           "a row that does not rescan behind a reset"}
    assert all(int(n) > 0 for n in caught.values()), caught
