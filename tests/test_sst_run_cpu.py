"""The rules of the device SST table reader (csrc/sst_run.h) on the CPU, no GPU: tests/cpp/sst_run_test.cc is the
control flow of the kernels of csrc/crc32c_sstindex.inc written lane by lane over a memory model, with every decision
taken from the header the kernels and the host forms themselves include.  Per emulated call the handles, the count and
the status equal a plain serial walk restated from table/block.cc (and Block::Iter's loop on a block with no error), at
cap below, at and above the count; every output element is written exactly once and nothing outside cap; every image
byte read lies inside the index block or the footer; no scratch word is read that the call did not write or written
past the runs the scratch holds.  Three deliberately wrong rules must be caught.  The program is built with
AddressSanitizer and UBSan and run as it is."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("sst_run") / "sst_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "sst_run_test.cc"), "-o", str(out)])
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=600)


def test_the_kernels_reproduce_the_serial_walk(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "PASS" in run.stdout and " 0 failed" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    # every block of up to 4 entries over 8 kinds at 3 intervals and 2-3 caps, the tail mutations, the restart counts
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 50000


def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"a run allowed to end past its end offset",
                           "shared unchecked on a run's first entry",
                           "the stop taken from the highest run with an error"}
    assert all(int(n) > 0 for n in caught.values()), caught


def test_kernels_and_host_forms_take_their_rules_from_the_header():
    """The kernels and the host forms keep no rule of their own: the footer, the tail, the run extents, the entry
    decode, the stop, the slot layout and the read check's prep come from sst_run.h, the file the program above
    includes; the pass uses no atomics and no memset, and the scan of the per-run counts is the offsets pass's own."""
    kernel = open(os.path.join(CSRC, "crc32c_sstindex.inc")).read()
    for call in ("sst::footer(", "sst::gate(", "sst::unmask(", "sst::count_lane(", "sst::Rule::stop_pick(",
                 "sst::stop_candidate(", "sst_stop_reduce(", "sst::keep_before(", "sst::fill_lane(", "sst::data_cap(", "sst::held(",
                 "sst::after_data(", "sst::final_status(", "sst::code_of(", "sst::listed(", "sst::prep(", "sst::le32("):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code and "0xdb47" not in code and "varint" not in code
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    walk = host[host.index("int launch_sst_walk_in("):host.index("int sst_walk_args(")]
    assert "launch_offsets_in(" in walk and "sst::pad_grid(" in walk and "sst::grid_for(" in walk
    assert "hipMemset" not in walk and "hipMalloc" not in walk
    body = host[host.index("int kvsep_sst_index_device("):host.index("// ---- the chains pass")]
    assert "hipMemset" not in body and "hipMalloc" not in body and "hipMemcpy" not in body
    assert "sst::scratch_words(" in host and "sst::runs_for(" in host
    framing = open(os.path.join(CSRC, "framing.cpp")).read()
    forms = framing[framing.index("int kvsep_sst_footer("):framing.index("uint64_t kvsep_log_accept(")]
    for call in ("sst::footer(", "sst::tail(", "sst::run_of(", "sst::walk_run(", "sst::held("):
        assert call in forms, call
    header = open(os.path.join(CSRC, "sst_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    assert "malloc" not in header and "new " not in re.sub(r"//.*", "", header)
