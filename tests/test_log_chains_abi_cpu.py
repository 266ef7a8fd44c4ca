"""The record-assembly entry points without a device: the three symbols are exported and bound, the ABI version is
still 4, the Context methods exist, and every argument refusal comes before any device (or the context) is touched --
so each fires here with a null ctx, or with a context pointer that is never dereferenced."""
import ctypes

import numpy as np
import pytest

import kvsep

NARGS = {"kvsep_log_chains": 7, "kvsep_log_chains_device": 15, "kvsep_log_records_device": 26}


@pytest.mark.parametrize("name", list(NARGS))
def test_exported_bound_and_in_the_header(name):
    assert hasattr(kvsep.lib(), name)
    res, args = kvsep._SIGS[name]
    assert res is (ctypes.c_uint64 if name == "kvsep_log_chains" else ctypes.c_int) and len(args) == NARGS[name]
    assert name in kvsep.header_functions()


def test_context_methods_and_host_binding():
    for m in ("log_chains_device", "log_records_device"):
        assert callable(getattr(kvsep.Context, m))
    first, whole, nchain, nwhole = kvsep.log_chains([2, 3, 4, 1, 3], [1, 1, 1, 1, 1])
    assert (first.tolist(), whole.tolist(), nchain, nwhole) == ([0, 3, 4, 5, 5, 5], [1, 1, 0, 0, 0], 3, 2)
    first, whole, nchain, nwhole = kvsep.log_chains([2, 3, 4, 1, 3], [1, 1, 1, 1, 1], gap=[0, 0, 1, 0, 0])
    assert (first.tolist(), whole.tolist(), nchain, nwhole) == ([0, 2, 3, 4, 5, 5], [0, 0, 1, 0, 0], 4, 1)
    first, whole, nchain, nwhole = kvsep.log_chains(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert (first.tolist(), whole.size, nchain, nwhole) == ([0], 0, 0, 0)


def test_abi_version_stays():
    assert kvsep.lib().kvsep_abi_version() == 4
    header = open(kvsep.HEADER_PATH).read()
    assert "#define KVSEP_ABI_VERSION 4" in header


def err():
    return kvsep.lib().kvsep_last_error().decode()


def test_chains_device_refusals_fire_without_a_device():
    L = kvsep.lib()
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    fake = p  # a context pointer: the refusals below come before it is looked at
    f = L.kvsep_log_chains_device
    assert f(None, None, p, p, None, None, None, p, 1, p, p, None, None, p, None) == -1 and "null ctx" in err()
    for missing in (2, 3, 9, 10):  # type, accept, first, whole
        args = [fake, None, p, p, None, None, None, p, 1, p, p, None, None, p, None]
        args[missing] = None
        assert f(*args) == -1 and "with cap != 0" in err(), missing
    for given in ((5,), (5, 6), (5, 6, 11), (12,)):  # some but not all of off, len, frag_off, frag_len
        args = [fake, None, p, p, None, None, None, p, 1, p, p, None, None, p, None]
        for k in given:
            args[k] = p
        assert f(*args) == -1 and "go together" in err(), given
    assert f(fake, None, p, p, None, None, None, None, 1, p, p, None, None, p, None) == -1 and "null nrec" in err()
    assert f(fake, None, p, p, None, None, None, p, 1, p, p, None, None, None, None) == -1 and "null nchain" in err()
    assert f(fake, None, p, p, None, None, None, p, 1 << 32, p, p, None, None, p, None) == -1 and "2^32" in err()
    assert all(w == 0 for w in word)


def test_records_device_refusals_fire_without_a_device():
    L = kvsep.lib()
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    f = L.kvsep_log_records_device

    def args(ctx=p, cap=1, **null):
        a = dict(ctx=ctx, stream=None, base=p, n=8, off=p, len=p, stored=p, type=p, ok=p, accept=p, gap=p, cap=cap,
                 nrec=p, dropped=None, bad_length=None, frag_off=p, frag_len=p, first=p, whole=p, nchain=p, dst=p,
                 dst_bytes=8, rec_off=p, rec_len=None, end=p, nwhole=None)
        for k in null:
            a[k] = None
        return list(a.values())

    assert f(*args(ctx=None)) == -1 and "null ctx" in err()
    for name in ("off", "len", "type", "ok", "accept", "stored", "gap", "frag_off", "frag_len", "first", "whole", "dst",
                 "rec_off"):
        assert f(*args(**{name: None})) == -1 and "null" in err(), name
    assert f(*args(nrec=None)) == -1 and "null nrec" in err()
    assert f(*args(nchain=None)) == -1 and "null nchain" in err()
    assert f(*args(end=None)) == -1 and "null end" in err()
    assert f(*args(base=None)) == -1 and "null base" in err()
    assert f(*args(cap=1 << 32)) == -1 and "2^32" in err()
    assert all(w == 0 for w in word)
