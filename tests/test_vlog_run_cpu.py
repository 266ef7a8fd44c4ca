"""The rules of the device value-log reader (csrc/vlog_run.h) on the CPU, no GPU:
tests/cpp/vlog_run_test.cc is the control flow of the two kernels of csrc/crc32c_vlogwalk.inc written lane by lane over
a memory model, with every decision taken from the header the kernels themselves include -- built with a 64-byte window,
so that every refill edge is reached in images of a few hundred bytes.  Per emulated call the walk's arrays, *nrec and
*consumed equal a plain serial walk and the totals a plain serial verdict loop, at cap below, at and above the count and
0, for a base of each of the 16 alignments; every load is an aligned 16-byte granule that holds a byte of the image;
every array element in [0, cap) is written exactly once and nothing past cap; the step counter never exceeds n / 8.
Three deliberately wrong rules must be caught.  The program also runs tests/golden/ref_small.vlog and every mutant of
the recorded vlog corpus (tests/golden/framing_corpus_vlog.json), with the expected arrays from the library's host
kvsep_vlog_walk.  The program is built with AddressSanitizer and UBSan and run as it is."""
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
WRONG = {"the payload test formed as p + 8 + l > n in 32 bits",
         "a header read from the window when only part of it is staged",
         "the store mask dropped at cap"}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("vlog_run") / "vlog_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKVSEP_VLOG_WINDOW=64",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "vlog_run_test.cc"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def run(program):
    return subprocess.run([program], capture_output=True, text=True, timeout=600)


def clean(r):
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout and " 0 failed" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_kernels_reproduce_the_serial_walk(run):
    clean(run)
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 10000


def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == WRONG
    assert all(int(n) > 0 for n in caught.values()), caught


def write_case(path, img):
    off, ln, stored, consumed = kvsep.vlog_walk(img)
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(img), off.size))
        f.write(img)
        for a, dt in ((off, np.uint64), (ln, np.uint64), (stored, np.uint32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        f.write(struct.pack("<Q", consumed))


def test_the_model_on_the_recorded_corpus(program, tmp_path_factory):
    """ref_small.vlog and every mutant of the vlog corpus: the image and the library's host walk go to a case file; the
    program checks its restated serial walk against it and the model against the walk, at cap = count - 1, count and
    count + 3, each at another alignment of the base."""
    doc, base = FC.load("vlog")
    d = tmp_path_factory.mktemp("vlog_cases")
    try:
        write_case(os.path.join(str(d), "0000.case"), base)
        k = 1
        for mutants in doc["classes"].values():
            for m in mutants:
                write_case(os.path.join(str(d), "%04d.case" % k), FC.mutate(base, m))
                k += 1
        r = subprocess.run([program, str(d)], capture_output=True, text=True, timeout=900)
    finally:
        shutil.rmtree(str(d), ignore_errors=True)
    clean(r)
    assert f"{k} case files" in r.stdout and k == 1 + sum(len(v) for v in doc["classes"].values()) == 280


def test_kernels_take_their_rules_from_the_header():
    """The kernels keep no rule of their own: the header and payload tests, the window's geometry, the refill rule, the
    emission batch, the padding and the totals come from vlog_run.h, the file the program above includes; the walk
    uses no atomics, no memset and no scratch, and the launch code allocates nothing."""
    kernel = open(os.path.join(CSRC, "crc32c_vlogwalk.inc")).read()
    for call in ("vlogrun::has_header(", "vlogrun::has_payload(", "vlogrun::header_len(", "vlogrun::header_stored(",
                 "vlogrun::rec_off(", "vlogrun::next_header(", "vlogrun::skew(", "vlogrun::window_hi(",
                 "vlogrun::granule_count(", "vlogrun::granule_addr(", "vlogrun::load_slot(", "vlogrun::load_granule(",
                 "vlogrun::slot_in_lds(", "vlogrun::staged(", "vlogrun::lds_index(", "vlogrun::lds_word(",
                 "vlogrun::header_of_words(", "vlogrun::emit_lane(", "vlogrun::batch_full(", "vlogrun::batch_first(",
                 "vlogrun::tail_count(", "vlogrun::emit_index(", "vlogrun::emit_store(", "vlogrun::pad_first(",
                 "vlogrun::good_count(", "vlogrun::has_good(", "vlogrun::has_drop(", "vlogrun::kPadStored"):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code and "16384" not in code
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    body = host[host.index("int launch_vlog_walk("):host.index("// ---- the SST table reader on the device")]
    assert "hipMemset" not in body and "hipMalloc" not in body and "hipStreamSynchronize" not in body
    assert "vlog_walk_kernel<<<1, vlogrun::kLanes" in body and "vlog_totals_kernel<<<1, vlogrun::kLanes" in body
    header = open(os.path.join(CSRC, "vlog_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    assert "constexpr uint64_t kHeader = 8;" in header
    assert int(re.search(r"constexpr uint32_t kPadStored = (0x[0-9a-f]+)u;", header).group(1), 16) == kvsep.mask(0)
