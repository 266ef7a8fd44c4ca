"""The rules of the device log / MANIFEST reader (csrc/log_run.h) on the CPU, no GPU:
tests/cpp/log_run_test.cc is the control flow of the six kernels of csrc/crc32c_logwalk.inc written lane by lane over a
memory model, with every decision taken from the header the kernels themselves include.  Per emulated call the walk's
arrays and *nrec equal a plain serial walk and accept / gap / dropped / bad-length bytes a plain serial accept loop, at
cap below, at and above the count; every output element is written exactly once and nothing outside cap; no image byte
outside [0, n) is read; no scratch word is read that the call did not write.  Three deliberately wrong rules must be
caught.  The program also runs every mutant of the recorded log corpus (tests/golden/framing_corpus_log.json), with the
expected arrays from the library's host kvsep_log_walk / kvsep_log_accept_gaps and the verdicts of its host leg -- the
model against recorded reference behaviour.  The program is built with AddressSanitizer and UBSan and run as it is."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kvsep
import framing_corpus as FC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("log_run") / "log_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "log_run_test.cc"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def run(program):
    return subprocess.run([program], capture_output=True, text=True, timeout=600)


def clean(r):
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout and " 0 failed" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_kernels_reproduce_the_serial_loops(run):
    clean(run)
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 500


def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"pending carried through a block that has records",
                           "a stop taken from a record in the dead part of its block",
                           "a bad length reported in a short last block"}
    assert all(int(n) > 0 for n in caught.values()), caught


def write_case(path, img, walk, ok):
    off, ln, stored, ty = walk
    accept, gap, dropped, bad_len = kvsep.log_accept_gaps(img, ok)
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(img), off.size))
        f.write(img)
        for a, dt in ((off, np.uint64), (ln, np.uint64), (stored, np.uint32), (ty, np.uint8), (ok, np.uint8),
                      (accept, np.uint8), (gap, np.uint8)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        f.write(struct.pack("<QQ", dropped, bad_len))


def test_the_model_on_the_recorded_corpus(program, tmp_path_factory):
    """Every mutant of the log corpus: the image, the library's host walk, the host leg's verdicts and the host accept
    outputs go to a case file; the program checks its restated serial loops against them and the model against the
    loops, at cap = count - 1, count and count + 3."""
    doc, base = FC.load("log")
    d = tmp_path_factory.mktemp("log_cases")
    try:
        k = 0
        for cls, mutants in doc["classes"].items():
            for m in mutants:
                img = FC.mutate(base, m)
                walk = kvsep.log_walk(img)
                ok = FC.log_host_ok(img, walk[0], walk[1], walk[2])
                FC.check_log(cls, m, img, doc["intact"], walk, ok)  # the expectations are the reference's own
                write_case(os.path.join(str(d), "%04d.case" % k), img, walk, ok)
                k += 1
        r = subprocess.run([program, str(d)], capture_output=True, text=True, timeout=900)
    finally:
        shutil.rmtree(str(d), ignore_errors=True)
    clean(r)
    assert f"{k} case files" in r.stdout and k == sum(len(v) for v in doc["classes"].values())


def test_kernels_take_their_rules_from_the_header():
    """The kernels keep no rule of their own: extents, the header classification, the search, the dead-block, stop and
    pending rules, the verdicts and the byte counts come from log_run.h, the file the program above includes; the pass
    uses no atomics and no memset, and the scan of the per-block counts is the offsets pass's own."""
    kernel = open(os.path.join(CSRC, "crc32c_logwalk.inc")).read()
    for call in ("logrun::block_begin(", "logrun::block_end(", "logrun::has_header(", "logrun::header_len(",
                 "logrun::classify(", "logrun::next_header(", "logrun::rec_off(", "logrun::rec_len(",
                 "logrun::header_stored(", "logrun::held(", "logrun::first_in_block(", "logrun::probe(",
                 "logrun::probe_right(", "logrun::in_block(", "logrun::after_record(", "logrun::dies(",
                 "logrun::stops(", "logrun::stop_min(", "logrun::block_pending(", "logrun::resolve(",
                 "logrun::bad_length_bytes(", "logrun::counts_bad_length(", "logrun::mismatch_bytes(",
                 "logrun::judge("):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code and "32768" not in code
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    walk = host[host.index("int launch_log_walk_in("):host.index("int launch_log_accept_in(")]
    assert "launch_offsets_in(" in walk and "logrun::pad_grid(" in walk
    body = host[host.index("int launch_log_walk_in("):host.index("template <typename Body>")]
    assert "hipMemset" not in body and "hipMalloc" not in body
    header = open(os.path.join(CSRC, "log_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    assert "constexpr uint64_t kBlock = 32768;" in header and "constexpr uint64_t kHeader = 7;" in header
