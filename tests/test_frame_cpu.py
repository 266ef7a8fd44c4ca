"""The device write side's entry points without a GPU: kvsep_crc32c_pack_device, kvsep_vlog_frame_offsets,
kvsep_vlog_frame_device and kvsep_sst_frame_device are declared, exported and bound; the offsets helper (host, pure)
equals a prefix sum and refuses what the vlog header cannot hold; the device calls refuse a null context before any
device is touched."""
import ctypes

import numpy as np
import pytest

import kvsep

NAMES = ["kvsep_crc32c_pack_device", "kvsep_vlog_frame_offsets", "kvsep_vlog_frame_device", "kvsep_sst_frame_device"]


def test_the_four_entry_points_are_declared_exported_and_bound():
    declared = kvsep.header_functions()
    l = ctypes.CDLL(kvsep.LIB_PATH)
    for n in NAMES:
        assert n in declared, n
        assert hasattr(l, n), n
        assert n in kvsep._SIGS, n
    for m in ("pack_device", "vlog_frame_device", "sst_frame_device"):
        assert callable(getattr(kvsep.Context, m))
    assert kvsep.lib().kvsep_abi_version() == 4  # new entry points only


def expected_offsets(lens, start):
    lens = np.asarray(lens, np.uint64)
    ends = np.uint64(start) + np.cumsum(lens + np.uint64(8), dtype=np.uint64)
    return np.concatenate([[np.uint64(start)], ends[:-1]]).astype(np.uint64) if lens.size else ends, \
        int(ends[-1]) if lens.size else start


@pytest.mark.parametrize("case", ["empty", "one", "random"])
def test_vlog_frame_offsets_is_the_prefix_sum(case):
    rng = np.random.default_rng(20261020)
    lens = {"empty": np.zeros(0, np.uint64), "one": np.array([4093], np.uint64),
            "random": rng.integers(0, 9000, 1000).astype(np.uint64)}[case]
    if case == "random":
        lens[[0, 17, 999]] = 0
    for start in (0, 12345, 2**40 + 3):
        off, end = kvsep.vlog_frame_offsets(lens, start)
        exp_off, exp_end = expected_offsets(lens, start)
        assert off.dtype == np.uint64 and np.array_equal(off, exp_off), (case, start)
        assert end == exp_end, (case, start)
    off, end = kvsep.vlog_frame_offsets(np.array([2**32 - 1, 0], np.uint64), 5)  # the longest payload the header holds
    assert off.tolist() == [5, 5 + 8 + 2**32 - 1] and end == 5 + 16 + 2**32 - 1


def test_vlog_frame_offsets_refuses_what_the_header_cannot_hold():
    with pytest.raises(kvsep.KvsepError):
        kvsep.vlog_frame_offsets(np.array([1, 2**32, 3], np.uint64))
    with pytest.raises(kvsep.KvsepError):  # the sum leaves 64 bits
        kvsep.vlog_frame_offsets(np.array([100, 100], np.uint64), 2**64 - 150)
    off, end = kvsep.vlog_frame_offsets(np.array([100], np.uint64), 2**64 - 150)  # ... and just does not
    assert off.tolist() == [2**64 - 150] and end == 2**64 - 42
    lens = np.array([1], np.uint64)
    vp = ctypes.c_void_p
    assert kvsep.lib().kvsep_vlog_frame_offsets(None, 1, 0, lens.ctypes.data_as(vp), None) == -1
    assert kvsep.lib().kvsep_vlog_frame_offsets(lens.ctypes.data_as(vp), 1, 0, None, None) == -1
    assert kvsep.lib().kvsep_vlog_frame_offsets(None, 0, 7, None, None) == 0


def test_a_null_context_is_refused_before_any_device_is_touched():
    l = kvsep.lib()
    assert l.kvsep_crc32c_pack_device(None, None, None, None, None, None, None, 0, None, 0, 0) == -1
    assert "null ctx" in l.kvsep_last_error().decode()
    assert l.kvsep_vlog_frame_device(None, None, None, None, None, None, None, None, None, 0, None, 0, 0, 0, 0) == -1
    assert "null ctx" in l.kvsep_last_error().decode()
    assert l.kvsep_sst_frame_device(None, None, None, None, None, None, None, None, 0, None, 0, 0, 0) == -1
    assert "null ctx" in l.kvsep_last_error().decode()
