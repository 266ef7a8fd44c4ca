"""The geometry of crc32c_pack_kernel (csrc/pack_run.h) on the CPU, no GPU and no library:
tests/cpp/pack_run_test.cc is the kernel's control flow written lane by lane over a memory model, with every index and
byte decision taken from the header the kernel itself includes.  Per emulated launch every destination byte of a block
that fits is written exactly once and no other, the destination equals memcpy, every load is a 16-B granule or a byte
that holds a segment byte, and the descriptor arrays are read inside their bounds -- for every source alignment x
destination alignment x length 0..80 and around the tile size, runs with zero-length segments, malformed first[], and
the fit predicate at its edges and near 2^64.  The program is built with AddressSanitizer and UBSan and run as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("pack_run") / "pack_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pack_run_test.cc"), "-o", str(out)])
    return str(out)


def test_geometry_partitions_and_reproduces_memcpy(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout and " 0 failed" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_kernel_takes_its_geometry_from_the_header():
    """The kernel keeps no index arithmetic of its own: the clamp, the fit, the tiles, the cuts, the edges, the body
    granules and the byte-align come from pack_run.h, the file the program above includes."""
    kernel = open(os.path.join(CSRC, "crc32c_pack.inc")).read()
    for call in ("pack::clamp_run(", "pack::add_sat(", "pack::fits(", "pack::tile_count(", "pack::tile_range(",
                 "pack::first_tile(", "pack::cut_segment(", "pack::pass_segs(", "pack::split(", "pack::edge_byte(",
                 "pack::body_iters(", "pack::body_granule(", "pack::body_src(", "pack::align16(",
                 "pack::vlog_header_byte(", "pack::sst_trailer_byte("):
        assert call in kernel, call
    host = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    assert "pack::team_size(" in host and "pack::chunk_count(" in host
    header = open(os.path.join(CSRC, "pack_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
