"""The geometry of the offsets pass (csrc/offsets_run.h) on the CPU, no GPU and no library:
tests/cpp/offsets_run_test.cc is the control flow of offsets_tile_sum_kernel, offsets_tile_scan_kernel and
offsets_write_kernel written lane by lane over a memory model, with every index and arithmetic decision taken from the
header the kernels themselves include.  Per emulated launch dst_off, *end and *nkept equal a plain serial loop, dst_off
is written once per block and nothing around it, seg_len / first / keep are read inside their bounds, and no scratch
word is read that the launch did not write -- for every count 0..70 and 1,020..1,030, all three keep rules, every
first[] of a small alphabet (decreasing and oversized values included), long runs, 257 tiles, and sums that reach
2^64.  Three deliberately wrong rules must be caught, and kSkip must be refused by pack::fits.  The program is built
with AddressSanitizer and UBSan and run as it is."""
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
    out = tmp_path_factory.mktemp("offsets_run") / "offsets_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "offsets_run_test.cc"), "-o", str(out)])
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=600)


def test_the_three_kernels_reproduce_the_serial_loop(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "PASS" in run.stdout and " 0 failed" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]


def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"an inclusive scan", "the keep mask ignored in the tile total", "an unclamped first[]"}
    assert all(int(n) > 0 for n in caught.values()), caught


def test_kernels_take_their_geometry_from_the_header():
    """The kernels keep no index arithmetic of their own: block indices, the clamp, the keep rule, sizes and extents,
    the scan steps, the per-thread runs and the placement come from offsets_run.h, the file the program above
    includes; and the pass uses no atomics and no memset."""
    kernel = open(os.path.join(CSRC, "crc32c_offsets.inc")).read()
    for call in ("offsets::block_index(", "offsets::clamp_run(", "offsets::is_kept(", "offsets::is_short(",
                 "offsets::long_iters(", "offsets::long_seg(", "offsets::block_size(", "offsets::extent(",
                 "offsets::add_sat(", "offsets::scan_shift(", "offsets::scan_takes(", "offsets::row_base(",
                 "offsets::scan_run(", "offsets::scan_range(", "offsets::place(", "offsets::layout_end("):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    assert "offsets::tile_count(" in host
    launch = host[host.index("int launch_offsets_in("):host.index("template <typename Then>")]
    assert "hipMemset" not in launch and "hipMalloc" not in launch
    header = open(os.path.join(CSRC, "offsets_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    assert "constexpr uint32_t kTile = 1024;" in header and "kSkip = ~uint64_t(0)" in header
