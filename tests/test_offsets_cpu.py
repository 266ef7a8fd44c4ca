"""The offsets and salvage entry points without a GPU: kvsep_crc32c_offsets_device, kvsep_crc32c_salvage_device,
kvsep_sst_salvage_device and kvsep_vlog_frame_auto_device are declared, exported and bound with the header's argument
lists; their argument refusals hold before any device is touched; the ABI version stays 4."""
import ctypes
import re

import kvsep

NAMES = ["kvsep_crc32c_offsets_device", "kvsep_crc32c_salvage_device", "kvsep_sst_salvage_device",
         "kvsep_vlog_frame_auto_device"]


def test_the_entry_points_are_declared_exported_and_bound():
    declared = kvsep.header_functions()
    l = ctypes.CDLL(kvsep.LIB_PATH)
    for n in NAMES:
        assert n in declared, n
        assert hasattr(l, n), n
        assert n in kvsep._SIGS, n
    for m in ("offsets_device", "salvage_device", "sst_salvage_device", "vlog_frame_auto_device"):
        assert callable(getattr(kvsep.Context, m))
    assert kvsep.OFFSET_SKIP == 2**64 - 1


def test_the_abi_version_is_still_4():
    assert kvsep.lib().kvsep_abi_version() == 4  # new entry points only
    header = open(kvsep.HEADER_PATH).read()
    assert "#define KVSEP_ABI_VERSION 4" in header and "#define KVSEP_OFFSET_SKIP UINT64_MAX" in header


def test_the_binding_has_the_header_argument_lists():
    """Every parameter of the header's declaration against the ctypes signature: pointers as c_void_p, uint64_t as
    c_uint64, in order."""
    src = re.sub(r"/\*.*?\*/", "", open(kvsep.HEADER_PATH).read(), flags=re.S)
    for n in NAMES:
        params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, src, flags=re.S).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else ctypes.c_uint64 for p in params]
        assert all("*" in p or "uint64_t" in p for p in params), (n, params)
        res, args = kvsep._SIGS[n]
        assert res is ctypes.c_int and args == want, n


P = 0x1000  # a non-null address that is never dereferenced: every call below is refused first


def err():
    return kvsep.lib().kvsep_last_error().decode()


def test_offsets_refusals():
    f = kvsep.lib().kvsep_crc32c_offsets_device
    #        ctx  stream seg_len first keep keep_before head tail start dst_off end nkept count nseg
    assert f(None, None, P, None, P, P, 0, 0, 0, P, P, None, 1, 1) == -1
    assert "both keep and keep_before" in err()
    assert f(None, None, P, None, None, None, 0, 0, 0, P, P, None, 2**32, 1) == -1
    assert "2^32 - 1 blocks" in err()
    assert f(None, None, P, None, None, None, 0, 0, 0, None, P, None, 1, 1) == -1 and "null dst_off or end" in err()
    assert f(None, None, P, None, None, None, 0, 0, 0, P, None, None, 0, 0) == -1 and "null dst_off or end" in err()
    assert f(None, None, None, None, None, None, 0, 0, 0, P, P, None, 1, 1) == -1 and "null seg_len" in err()
    assert f(None, None, P, None, P, None, 0, 0, 0, P, P, None, 2**32 - 1, 1) == -1 and "null ctx" in err()
    assert f(None, None, None, None, None, None, 8, 5, 7, None, P, None, 0, 0) == -1 and "null ctx" in err()


def test_salvage_refusals():
    l = kvsep.lib()
    f = l.kvsep_crc32c_salvage_device
    #        ctx  stream base off len keep keep_before dst dst_bytes dst_off end nkept count
    assert f(None, None, P, P, P, P, P, P, 64, P, P, None, 1) == -1 and "both keep and keep_before" in err()
    assert f(None, None, P, P, P, None, None, P, 64, P, P, None, 2**32) == -1 and "2^32 - 1 blocks" in err()
    assert f(None, None, P, P, P, None, P, P, 64, P, None, None, 1) == -1 and "null dst_off or end" in err()
    assert f(None, None, P, P, None, None, P, P, 64, P, P, None, 1) == -1 and "null off, len or dst" in err()
    assert f(None, None, P, P, P, None, P, P, 64, P, P, None, 1) == -1 and "null ctx" in err()
    g = l.kvsep_sst_salvage_device
    #        ctx  stream file off len out first_bad nbad ok dst dst_bytes dst_off end nkept count total max_len
    assert g(None, None, P, P, P, P, None, None, P, P, 64, P, P, None, 2**32, 0, 0) == -1 and "2^32 - 1 blocks" in err()
    assert g(None, None, P, P, P, P, None, None, None, P, 64, P, P, None, 1, 0, 0) == -1 and "null argument" in err()
    assert g(None, None, P, P, P, P, None, None, P, P, 64, P, None, None, 1, 0, 0) == -1 and "null dst_off or end" in err()
    assert g(None, None, P, P, P, P, None, None, P, P, 64, P, P, None, 1, 0, 0) == -1 and "null ctx" in err()
    h = l.kvsep_vlog_frame_auto_device
    #        ctx  stream base seg_off seg_len first seg_crc crc_out dst dst_bytes start rec_off end count nseg total max
    assert h(None, None, P, P, P, P, P, P, P, 64, 0, None, P, 1, 1, 0, 0) == -1 and "null dst_off or end" in err()
    assert h(None, None, P, P, P, P, P, P, P, 64, 0, P, P, 2**32, 1, 0, 0) == -1 and "2^32 - 1 blocks" in err()
    assert h(None, None, P, P, P, P, P, P, P, 64, 0, P, P, 1, 1, 0, 0) == -1 and "null ctx" in err()
