"""The device log / MANIFEST reader's entry points without a device: the three symbols are exported and bound, the
Context methods exist, and the argument refusals come before any device is touched (a null ctx returns KVSEP_EINVAL)."""
import ctypes

import pytest

import kvsep

NAMES = ("kvsep_log_walk_device", "kvsep_log_accept_gaps_device", "kvsep_log_read_device")
NARGS = {"kvsep_log_walk_device": 10, "kvsep_log_accept_gaps_device": 14, "kvsep_log_read_device": 15}


@pytest.mark.parametrize("name", NAMES)
def test_exported_bound_and_in_the_header(name):
    assert hasattr(kvsep.lib(), name)
    res, args = kvsep._SIGS[name]
    assert res is ctypes.c_int and len(args) == NARGS[name]
    assert name in kvsep.header_functions()


def test_context_methods():
    for m in ("log_walk_device", "log_accept_gaps_device", "log_read_device"):
        assert callable(getattr(kvsep.Context, m))


def test_abi_version_stays():
    assert kvsep.lib().kvsep_abi_version() == 4


def test_null_ctx_is_refused_before_any_device():
    L = kvsep.lib()
    word = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.kvsep_log_walk_device(None, None, p, 8, None, None, None, None, 0, p) == -1
    assert "null ctx" in kvsep.lib().kvsep_last_error().decode()
    assert L.kvsep_log_accept_gaps_device(None, None, p, 8, p, p, p, p, p, 1, p, None, None, None) == -1
    assert "null ctx" in kvsep.lib().kvsep_last_error().decode()
    assert L.kvsep_log_read_device(None, None, p, 8, p, p, p, p, p, p, None, 1, p, None, None) == -1
    assert "null ctx" in kvsep.lib().kvsep_last_error().decode()
