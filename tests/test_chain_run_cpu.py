"""The rules of the chains pass (csrc/chain_run.h) on the CPU, no GPU: which physical records of a log / MANIFEST join
into the logical records log::Reader::ReadRecord returns.

tests/cpp/chain_run_test.cc is the control flow of the three kernels of csrc/crc32c_logchain.inc written lane by lane
over a memory model, with every decision taken from the header the kernels and kvsep_log_chains include, against the
documented assembly loop restated serially: every output element written exactly once, nothing outside cap (cap + 1
for first), no scratch word read that the call did not write, and three deliberately wrong rules caught.  The program is
built with AddressSanitizer and UBSan and run as it is.  The host function kvsep_log_chains is held to the recorded
reference: on every mutant of the log corpus the fragments of its whole chains, concatenated, are the records
log::Reader returned; and to a Python restatement of the rule table on random triples."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kvsep
import framing_corpus as FC
from framing_builders import FIRST, FULL, LAST, MIDDLE, assemble, fnv64
from framing_builders import log_chain_table as table

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("chain_run") / "chain_run_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "chain_run_test.cc"), "-o", str(out)])
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=900)


@needs_gxx
def test_the_kernels_reproduce_the_documented_loop(run):
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "PASS" in run.stdout and " 0 failed" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert int(re.search(r"(\d+) emulated calls", run.stdout).group(1)) >= 500


@needs_gxx
def test_the_model_catches_each_wrong_rule(run):
    caught = dict(re.findall(r"wrong rule \((.+?)\): caught in (\d+) cases", run.stdout))
    assert set(caught) == {"gap ignored on a LAST", "a tile of only KEEP ops that resets the incoming state",
                           "a FIRST that continues the chain before it"}
    assert all(int(n) > 0 for n in caught.values()), caught


def records_of(img, off, ln, first, whole, nchain):
    """[[len, fnv64], ...] of the whole chains' fragments, concatenated."""
    out = []
    for j in range(nchain):
        if whole[j]:
            r = b"".join(img[int(off[i]) + 1:int(off[i]) + int(ln[i])] for i in range(int(first[j]), int(first[j + 1])))
            out.append([len(r), fnv64(r)])
    return out


def test_log_chains_on_the_recorded_corpus():
    """Every mutant: the host walk, the host leg's verdicts, kvsep_log_accept_gaps, then kvsep_log_chains.  The
    fragments of each whole chain give exactly the records log::Reader returned, which is also what the documented
    loop (framing_builders.assemble) gives."""
    doc, base = FC.load("log")
    k = 0
    for cls, mutants in doc["classes"].items():
        for m in mutants:
            what = FC.describe(cls, m)
            img = FC.mutate(base, m)
            off, ln, stored, ty = kvsep.log_walk(img)
            ok = FC.log_host_ok(img, off, ln, stored)
            accept, gap, _, _ = kvsep.log_accept_gaps(img, ok)
            first, whole, nchain, nwhole = kvsep.log_chains(ty, accept, gap)
            got = records_of(img, off, ln, first, whole, nchain)
            diff = FC.first_difference(got, FC.want_records(m, doc["intact"]))
            assert diff is None, f"{what}: {diff}"
            assert got == assemble(img, off, ln, ty, accept, gap), what
            assert nwhole == len(got) and (first[nchain:] == off.size).all() and not whole[nchain:].any(), what
            k += 1
    assert k == sum(len(v) for v in doc["classes"].values()) and k > 100


def test_log_chains_against_the_table_on_random_triples():
    rng = np.random.default_rng(20261020)
    for k in range(2000):
        n = int(rng.integers(0, 301))
        ty = rng.choice(np.array([FULL, FIRST, MIDDLE, MIDDLE, MIDDLE, LAST, 0, 5], np.uint8), n)
        accept = (rng.random(n) < (0.9 if k % 2 else 0.6)).astype(np.uint8)
        gap = (rng.random(n) < (0.05 if k % 3 else 0.4)).astype(np.uint8)
        first, whole, nchain, nwhole = kvsep.log_chains(ty, accept, None if k % 5 == 0 else gap)
        if k % 5 == 0:
            gap[:] = 0
        wf, ww, wn = table(ty, accept, gap)
        assert (first.tolist(), whole.tolist(), nchain, nwhole) == (wf, ww, wn, sum(ww)), (k, n)
        # a synthetic image: record i's payload is 1 + i % 5 bytes of its own index at off[i] + 1
        ln = np.array([2 + i % 5 for i in range(n)], np.uint64)
        off = np.concatenate(([0], np.cumsum(ln)[:-1])).astype(np.uint64) if n else np.zeros(0, np.uint64)
        img = b"".join(bytes([0xEE]) + bytes([i & 0xFF]) * (1 + i % 5) for i in range(n))
        assert records_of(img, off, ln, first, whole, nchain) == assemble(img, off, ln, ty, accept, gap), (k, n)


def test_kernels_and_host_take_their_rules_from_the_header():
    """The kernels and kvsep_log_chains keep no rule of their own: the op of a record, the composition, `continues`,
    the chain-end test, the row resolution, the tile summary, the scan runs, the fragment descriptors and the padding
    come from chain_run.h, the file the program above includes; the pass uses no atomics and no memset."""
    kernel = open(os.path.join(CSRC, "crc32c_logchain.inc")).read()
    for call in ("chain::held(", "chain::op_of(", "chain::compose(", "chain::apply(", "chain::continues(",
                 "chain::next_index(", "chain::chain_ends(", "chain::whole_end(", "chain::row_op(",
                 "chain::state_before(", "chain::state_after_row(", "chain::lanes_below(", "chain::then(",
                 "chain::empty_summary(", "chain::pack_summary(", "chain::unpack_summary(", "chain::pack_in(",
                 "chain::in_state(", "chain::in_base(", "chain::chain_of(", "chain::block_index(", "chain::frag_off(",
                 "chain::frag_len(", "chain::pads_first(", "chain::pads_whole(", "chain::pads_frag(",
                 "chain::pad_first(", "offsets::scan_run(", "offsets::scan_range("):
        assert call in kernel, call
    assert "atomic" not in kernel and "hipMemset" not in kernel
    code = re.sub(r"//.*", "", kernel)
    for rule in ("kFirst", "kMiddle", "kLast", "kFull", "== 2", "== 3", "== 4"):
        assert rule not in code, rule
    host = open(os.path.join(CSRC, "framing.cpp")).read()
    body = host[host.index("uint64_t kvsep_log_chains("):]
    for call in ("chain::continues(", "chain::apply(", "chain::op_of(", "chain::next_index(", "chain::chain_ends(",
                 "chain::whole_end(", "chain::pads_first(", "chain::pads_whole(", "chain::pad_first("):
        assert call in body, call
    assert "kFirst" not in body and "kLast" not in body
    launch = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    launch = launch[launch.index("int launch_chains_in("):launch.index("int kvsep_log_records_device(")]
    assert "hipMemset" not in launch and "hipMalloc" not in launch
    assert "chain::tile_count(" in launch and "chain::write_tiles(" in launch
    header = open(os.path.join(CSRC, "chain_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
