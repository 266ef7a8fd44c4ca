"""The log write-side entry points without a device: the two symbols are exported and bound, the ABI version is still
4, every argument refusal of kvsep_log_frame_device comes before any device (or the context) is touched, and the pure
host function kvsep_log_frame_layout gives the offsets log::Writer::AddRecord gives -- on random record lists, on the 12
records of the committed reference MANIFEST and across a reopen at every record boundary."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import kvsep
from framing_builders import BLOCK, log_image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "kv-separate_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NARGS = {"kvsep_log_frame_layout": 8, "kvsep_log_frame_device": 21}
SKIP = 2**64 - 1


@pytest.mark.parametrize("name", list(NARGS))
def test_exported_bound_and_in_the_header(name):
    assert hasattr(kvsep.lib(), name)
    res, args = kvsep._SIGS[name]
    assert res is ctypes.c_int and len(args) == NARGS[name]
    assert name in kvsep.header_functions()
    assert callable(kvsep.Context.log_frame_device) and callable(kvsep.log_frame_layout)


def test_abi_version_stays():
    assert kvsep.lib().kvsep_abi_version() == 4
    assert "#define KVSEP_ABI_VERSION 4" in open(kvsep.HEADER_PATH).read()


def err():
    return kvsep.lib().kvsep_last_error().decode()


def test_frame_device_refusals_fire_without_a_device():
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    f = kvsep.lib().kvsep_log_frame_device

    def args(ctx=p, count=1, frag_cap=1, **null):
        a = dict(ctx=ctx, stream=None, base=p, off=p, len=p, keep=None, count=count, dest_length=0, dst=p, dst_bytes=8,
                 rec_at=p, frag_first=p, frag_off=p, frag_len=p, frag_at=p, frag_type=p, frag_crc=p, frag_cap=frag_cap,
                 nfrag=p, written=p, total_bytes=0)
        for k in null:
            a[k] = None
        return list(a.values())

    assert f(*args(ctx=None)) == -1 and "null ctx" in err()
    for name in ("base", "off", "len", "rec_at"):
        assert f(*args(**{name: None})) == -1 and "with count != 0" in err(), name
    for name in ("frag_off", "frag_len", "frag_at", "frag_type", "frag_crc", "dst"):
        assert f(*args(**{name: None})) == -1 and "with frag_cap != 0" in err(), name
    for name in ("frag_first", "nfrag", "written"):
        assert f(*args(**{name: None})) == -1 and "null frag_first, nfrag or written" in err(), name
    assert f(*args(count=1 << 32)) == -1 and "2^32" in err()
    assert f(*args(frag_cap=1 << 32)) == -1 and "2^32" in err()
    assert all(w == 0 for w in word)
    assert kvsep.lib().kvsep_log_frame_layout(None, None, 1, 0, None, p, None, None) == -1 and "null" in err()
    assert kvsep.lib().kvsep_log_frame_layout(None, None, 0, 0, None, None, None, None) == -1


class NoCrc:
    """framing_builders.log_image wants an oracle for its checksums; the layout needs none."""

    class lib:
        @staticmethod
        def oracle_crc32c_mask(x):
            return 0

    @staticmethod
    def extend(_crc, _data):
        return 0


def want_layout(lens, keep, dest_length):
    """(rec_at, frag_first, physical records, bytes appended) from log_image's `physical` list: the log so far is
    dest_length % 32768 bytes of one record that ends exactly there, the kept records follow."""
    b0 = dest_length % BLOCK
    recs = [bytes(b0 - 7)] if b0 >= 7 else []
    assert b0 == 0 or b0 >= 7
    recs += [bytes(int(n)) for n, k in zip(lens, keep) if k]
    img, phys = log_image(recs, NoCrc)
    phys = phys[1:] if b0 else phys
    rec_at, frag_first, f = [], [], 0
    for k in keep:
        frag_first.append(f)
        if not k:
            rec_at.append(SKIP)
            continue
        rec_at.append(phys[f][0] - b0)
        while True:  # FULL or LAST ends the record
            t = phys[f][1]
            f += 1
            if t in (1, 4):
                break
    frag_first.append(f)
    assert f == len(phys)
    return rec_at, frag_first, [(at - b0, t, n) for at, t, n in phys], len(img) - b0


def check(lens, keep, dest_length):
    rec_at, frag_first, nfrag, written = kvsep.log_frame_layout(lens, None if all(keep) else keep, dest_length)
    w_at, w_first, phys, w_written = want_layout(lens, keep, dest_length)
    assert rec_at.tolist() == w_at and frag_first.tolist() == w_first, (lens, keep, dest_length)
    assert (nfrag, written) == (len(phys), w_written), (lens, keep, dest_length)
    kept = sum(1 for k in keep if k)
    assert nfrag <= 2 * kept + sum(int(n) for n, k in zip(lens, keep) if k) // 32761  # the documented bound
    return phys


def test_layout_on_random_record_lists():
    rng = np.random.default_rng(20261020)
    for k in range(2000):
        n = int(rng.integers(0, 40))
        kind = k % 4
        if kind == 0:
            lens = rng.integers(0, 41, n)
        elif kind == 1:
            lens = rng.integers(4673, 4681, n)
        elif kind == 2:
            lens = rng.choice(np.array([0, 1, 6, 7, 8, 32753, 32754, 32760, 32761, 32762, 65521, 65522, 65523, 100000]), n)
        else:
            lens = rng.integers(0, 70000, n)
        keep = [1] * n if k % 3 else (rng.random(n) < 0.7).astype(int).tolist()
        b0 = 0 if k % 5 == 0 else int(rng.choice([7, 8, 32754, 32760, 32761, 32762, 32767, int(rng.integers(7, 32768))]))
        check(lens.tolist(), keep, b0 + BLOCK * (k % 3))


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "ref_framing.json")) as f:
        lg = json.load(f)["log"]
    with open(os.path.join(GOLDEN, "ref_manifest.log"), "rb") as f:
        return lg["lens"], f.read()


def walk_headers(img):
    """(header offset, type, payload length) of every physical record of an intact image."""
    off, ln, _, ty = kvsep.log_walk(img)
    return [(int(o) - 6, int(t), int(n) - 1) for o, n, t in zip(off, ln, ty)]


def test_layout_reproduces_the_reference_manifest(manifest):
    lens, img = manifest
    assert len(lens) == 12 and len(img) == 327720
    phys = check(lens, [1] * 12, 0)
    assert len(phys) == 19 and phys == walk_headers(img)


def test_layout_across_a_reopen_at_every_record_boundary(manifest):
    lens, img = manifest
    headers = walk_headers(img)
    for cut in range(13):
        at_a, first_a, nf_a, wr_a = kvsep.log_frame_layout(lens[:cut], dest_length=0)
        at_b, first_b, nf_b, wr_b = kvsep.log_frame_layout(lens[cut:], dest_length=wr_a)
        assert nf_a + nf_b == 19 and wr_a + wr_b == len(img), cut
        starts = at_a.tolist() + [wr_a + a for a in at_b.tolist()]
        firsts = first_a.tolist()[:-1] + [nf_a + f for f in first_b.tolist()]
        assert [headers[f][0] for f in firsts[:-1]] == starts, cut


def test_kernels_and_host_take_their_rules_from_the_header():
    """The kernels and kvsep_log_frame_layout keep no rule of their own: the writer's offset, the reduction, the row
    resolution, the fragment count and block advance, the fragment descriptors, the owner search and the padding come
    from logw_run.h, the file the CPU program includes; the pass uses no atomics and no memset."""
    kernel = open(os.path.join(CSRC, "crc32c_logframe.inc")).read()
    for call in ("logw::row_count(", "logw::step_of(", "logw::lanes_below(", "logw::raw_before(", "logw::raw_behind(",
                 "logw::resets(", "logw::commit_mask(", "logw::last_lane(", "logw::start_of(", "logw::nfrag(",
                 "logw::blocks_advanced(", "logw::laid(", "logw::frags_of(", "logw::rec_at(", "logw::pack_rec(",
                 "logw::pad_bytes(", "logw::rel(", "logw::pos_sat(", "logw::pads_frag(", "logw::owner(", "logw::rec_b(",
                 "logw::rec_pad(", "logw::frag_type(", "logw::frag_begin(", "logw::frag_len(", "logw::frag_at(",
                 "logw::seed_of(", "logw::writes_pad(", "logw::add_sat("):
        assert call in kernel, call
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "hipMemset" not in code
    for rule in ("32768", "32761", "32769", "kAvail", "kBlock", "kHeader", "kFull", "kFirst", "kMiddle", "kLast", "% "):
        assert rule not in code, rule
    host = open(os.path.join(CSRC, "framing.cpp")).read()
    body = host[host.index("int kvsep_log_frame_layout("):host.index("int kvsep_sst_trailers_host(")]
    for call in ("logw::start_state(", "logw::start_of(", "logw::nfrag(", "logw::blocks_advanced(", "logw::resets(",
                 "logw::raw_behind(", "logw::step_of(", "logw::laid(", "logw::rec_at(", "logw::frags_of(", "logw::rel(",
                 "logw::pos_sat("):
        assert call in body, call
    for rule in ("32768", "32761", "kLogBlock", "kLogHeader", "% "):
        assert rule not in body, rule
    launch = open(os.path.join(CSRC, "crc32c_device.hip")).read()
    launch = launch[launch.index("int kvsep_log_frame_device("):launch.index("int kvsep_sst_verify_device(")]
    assert "hipMemset" not in launch and "hipMalloc" not in launch
    assert "logw::fill_lanes(" in launch and "logw::start_state(" in launch and "32761" not in launch
    header = open(os.path.join(CSRC, "logw_run.h")).read()
    assert "#include <hip" not in header and "#include <cstdint>" in header
    pack = open(os.path.join(CSRC, "pack_run.h")).read()
    assert "kLog = 3" in pack and "log_header_byte(" in pack
