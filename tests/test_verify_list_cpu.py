"""The list forms of the verify calls refuse bad arguments before any device is touched.  No GPU.

kvsep_crc32c_verify_list_device, kvsep_sst_verify_list_device, kvsep_sst_verify_list_host, kvsep_log_verify_device and
kvsep_crc32c_group_verify_list_device (include/kvsep_crc32c.h): a null context (group), or a null bad_idx with
bad_cap > 0, is KVSEP_EINVAL, and kvsep_last_error() names the function that refused."""
import ctypes

import pytest

import kvsep

EINVAL = -1
P = ctypes.c_void_p
CTX = P(0x1000)  # never dereferenced: every call below is refused on its arguments alone


def call(name, *args):
    rc = getattr(kvsep.lib(), name)(*args)
    return rc, kvsep.lib().kvsep_last_error().decode()


def verify_list(ctx, bad_idx, bad_cap):
    buf = (ctypes.c_uint32 * 4)()
    return call("kvsep_crc32c_verify_list_device", ctx, None, buf, buf, buf, None, buf, buf, None, None, bad_idx,
                bad_cap, None, 1, 4, 4)


def sst_list_device(ctx, bad_idx, bad_cap):
    buf = (ctypes.c_uint32 * 4)()
    return call("kvsep_sst_verify_list_device", ctx, None, buf, buf, buf, buf, None, None, bad_idx, bad_cap, None, 1,
                4, 4)


def sst_list_host(ctx, bad_idx, bad_cap):
    img = (ctypes.c_uint8 * 16)()
    off, ln = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(4)
    out = (ctypes.c_uint32 * 1)()
    return call("kvsep_sst_verify_list_host", ctx, img, 16, off, ln, out, None, None, bad_idx, bad_cap, 1)


def log_device(ctx):
    buf = (ctypes.c_uint32 * 4)()
    return call("kvsep_log_verify_device", ctx, None, buf, buf, buf, buf, buf, 1, 4, 4)


def group_list(g, bad_idx, bad_cap):
    one = (P * 1)(0)
    u = (ctypes.c_uint64 * 1)(1)
    res = (ctypes.c_uint64 * 2)()
    return call("kvsep_crc32c_group_verify_list_device", g, one, one, one, None, one, one, u, u, u, u, res,
                ctypes.byref(res, 8), bad_idx, bad_cap)


LIST_FORMS = {
    "kvsep_crc32c_verify_list_device": verify_list,
    "kvsep_sst_verify_list_device": sst_list_device,
    "kvsep_sst_verify_list_host": sst_list_host,
    "kvsep_crc32c_group_verify_list_device": group_list,
}


@pytest.mark.parametrize("name", sorted(LIST_FORMS))
def test_null_context_is_refused(name):
    some = (ctypes.c_uint64 * 4)()
    rc, err = LIST_FORMS[name](None, some, 4)
    assert rc == EINVAL and name in err, (rc, err)


@pytest.mark.parametrize("name", sorted(LIST_FORMS))
def test_null_bad_idx_with_a_capacity_is_refused(name):
    rc, err = LIST_FORMS[name](CTX, None, 1)
    assert rc == EINVAL and name in err and "bad_idx" in err, (rc, err)


def test_log_verify_device_refuses_a_null_context():
    rc, err = log_device(None)
    assert rc == EINVAL and "kvsep_log_verify_device" in err, (rc, err)


def test_the_binding_has_the_list_forms():
    for name in list(LIST_FORMS) + ["kvsep_log_verify_device"]:
        assert name in kvsep._SIGS and name in kvsep.header_functions(), name
    for cls, method in ((kvsep.Context, "verify_list_device"), (kvsep.Context, "sst_verify_list_device"),
                        (kvsep.Context, "sst_verify_list"), (kvsep.Context, "log_verify_device"),
                        (kvsep.Group, "verify_list_device")):
        assert callable(getattr(cls, method)), method
    assert kvsep.lib().kvsep_abi_version() == 4  # new entry points only: the version stays
