"""The rules of the device SST table writer (csrc/sstw_run.h) on the CPU, no GPU: tests/cpp/sstw_run_test.cc is the
control flow of the size, fill and tail kernels of csrc/crc32c_sstbuild.inc written lane by lane over a memory model,
with every decision taken from the header the kernels and the host forms themselves include.  Per emulated call the
output equals BlockBuilder::Add / Finish and Footer::EncodeTo restated serially; every destination byte of the range is
written exactly once and none outside it; every key byte read lies inside a kept key; a refusal writes nothing.  Three
deliberately wrong rules must be caught.  The program is built with AddressSanitizer and UBSan and run as it is."""
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
    out = tmp_path_factory.mktemp("sstw_run") / "sstw_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "sstw_run_test.cc"), "-o", str(out)])
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=600)


def test_the_kernels_reproduce_the_serial_block_builder(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "PASS" in run.stdout and " 0 failed" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    # 7 counts x 6 masks x 2 forms, the widths, 16 x 16 alignments x 2, the room
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 600


def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"a restart array with no entry for the empty block",
                           "a rank taken from the entry index",
                           "an edge written with a 16-B store"}
    assert all(int(n) > 0 for n in caught.values()), caught


def test_kernels_and_host_forms_take_their_rules_from_the_header():
    """The kernels and the host forms keep no rule of their own; the pass uses no atomics and no memset, and the two
    exclusive sums are the offsets pass's own."""
    kernel = open(os.path.join(CSRC, "crc32c_sstbuild.inc")).read()
    for call in ("sst::count_lane_keys(", "sst::fill_lane_keys(", "sstw::plan(", "sstw::kept(", "sstw::entry_size(",
                 "sstw::stages(", "sstw::split(", "sstw::edge_index(", "sstw::head_byte(", "sstw::value_byte(",
                 "sstw::frame_byte(", "sstw::restart_at(", "sstw::count_at(", "sstw::count_word(",
                 "sstw::lone_restart(", "sstw::trailer_byte(", "sstw::meta_byte(", "sstw::footer_byte(",
                 "sstw::table_bytes(", "sstw::refuses("):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code and "0xdb47" not in code and "varint" not in code
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    build = host[host.index("int launch_sst_build_in("):host.index("int kvsep_sst_index_device(")]
    assert build.count("launch_offsets_in(") == 2 and "launch_batch_in(" in build and "sstw::slices(" in build
    body = host[host.index("int launch_sst_build_in("):host.index("// ---- the chains pass")]
    assert "hipMemset" not in body and "hipMalloc" not in body and "hipMemcpy" not in body
    assert "sstw::scratch_words(" in host
    framing = open(os.path.join(CSRC, "framing.cpp")).read()
    forms = framing[framing.index("int kvsep_sst_index_keys("):framing.index("uint64_t kvsep_log_accept(")]
    for call in ("sst::walk_run_keys(", "sstw::plan(", "sstw::entry_size(", "sstw::frame_byte(", "sstw::restart_at(",
                 "sstw::count_at(", "sstw::lone_restart(", "sstw::trailer_byte(", "sstw::footer_byte("):
        assert call in forms, call
    header = open(os.path.join(CSRC, "sstw_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    assert "malloc" not in header and "new " not in re.sub(r"//.*", "", header)
