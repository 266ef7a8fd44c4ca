"""The SST table reader's host forms against the reference's own file, and its entry points without a device:
kvsep_sst_footer and kvsep_sst_index_walk on tests/golden/ref_table.sst give the handles the reference recorded in
ref_framing.json; the test table writer (sst_tables.py) reproduces the golden index block byte for byte from its keys
and handles, which pins the synthetic tables of the other tests to the reference's format; the four symbols are
exported with ABI 4; the argument refusals come before the context or a device is touched."""
import ctypes
import json
import os

import numpy as np
import pytest

import kvsep
import sst_tables as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NARGS = {"kvsep_sst_footer": 4, "kvsep_sst_index_walk": 7, "kvsep_sst_index_device": 10,
         "kvsep_sst_table_verify_device": 17}


@pytest.fixture(scope="module")
def golden_table():
    with open(os.path.join(GOLDEN, "ref_table.sst"), "rb") as f:
        img = f.read()
    with open(os.path.join(GOLDEN, "ref_framing.json")) as f:
        blocks = json.load(f)["sst"]["blocks"]
    return img, blocks


def test_footer_of_the_reference_table(golden_table):
    img, blocks = golden_table
    handles, status = kvsep.sst_footer(img)
    assert status == kvsep.SST_OK and handles == (214157, 8, 214170, 1185)
    assert [list(handles[:2]), list(handles[2:])] == [b[:2] for b in blocks[52:]]


def test_index_walk_of_the_reference_table(golden_table):
    img, blocks = golden_table
    (_, _, ioff, ilen), _ = kvsep.sst_footer(img)
    off, ln, nblocks, status = kvsep.sst_index_walk(img[ioff:ioff + ilen])
    assert (nblocks, status) == (52, kvsep.SST_OK)
    assert [[int(o), int(k)] for o, k in zip(off, ln)] == [b[:2] for b in blocks[:52]]


@pytest.mark.parametrize("cap", [0, 1, 51, 52, 60])
def test_cap_cuts_the_arrays_and_not_the_count(golden_table, cap):
    img, blocks = golden_table
    (_, _, ioff, ilen), _ = kvsep.sst_footer(img)
    off, ln, nblocks, status = kvsep.sst_index_walk(img[ioff:ioff + ilen], cap=cap)
    assert (nblocks, status, off.size) == (52, kvsep.SST_OK, cap)
    m = min(cap, 52)
    assert [[int(o), int(k)] for o, k in zip(off[:m], ln[:m])] == [b[:2] for b in blocks[:m]]
    assert not off[m:].any() and not ln[m:].any()


def test_the_table_writer_reproduces_the_golden_index_block(golden_table):
    img, blocks = golden_table
    ioff, ilen = blocks[53][:2]
    block = img[ioff:ioff + ilen]
    keys, handles = T.parse_index(block)
    assert handles == [tuple(b[:2]) for b in blocks[:52]]
    assert T.index_block(keys, handles, 1) == block, "the reference writes index blocks at restart interval 1"
    assert T.trailer(block) == img[ioff + ilen:ioff + ilen + 5]
    assert T.footer(tuple(blocks[52][:2]), (ioff, ilen)) == img[-48:]
    for interval in (2, 16):  # other intervals hold the same entries
        again = T.index_block(keys, handles, interval)
        assert T.parse_index(again) == (keys, handles) and len(again) < len(block)
        off, ln, nblocks, status = kvsep.sst_index_walk(again)
        assert (nblocks, status) == (52, kvsep.SST_OK)
        assert list(zip(off.tolist(), ln.tolist())) == handles


@pytest.mark.parametrize("nblocks,interval", [(0, 1), (1, 1), (65, 1), (65, 16), (1025, 3)])
def test_synthetic_tables_walk_back(nblocks, interval):
    img, off, ln, meta, index = T.build_table(nblocks, interval)
    handles, status = kvsep.sst_footer(img)
    assert status == kvsep.SST_OK and handles == meta + index
    got_off, got_len, n, status = kvsep.sst_index_walk(img[index[0]:index[0] + index[1]].tobytes())
    assert (n, status) == (nblocks, kvsep.SST_OK)
    assert np.array_equal(got_off, off) and np.array_equal(got_len, ln)


def test_damaged_blocks_report_the_first_error(golden_table):
    img, blocks = golden_table
    ioff, ilen = blocks[53][:2]
    block = bytearray(img[ioff:ioff + ilen])
    keys, handles = T.parse_index(bytes(block))
    nr = int.from_bytes(block[-4:], "little")
    ro = len(block) - 4 * (1 + nr)
    restart = lambda r: int.from_bytes(block[ro + 4 * r:ro + 4 * r + 4], "little")
    hurt = bytearray(block)
    hurt[restart(30)] = 1  # shared = 1 on a run's first entry
    hurt[restart(10) + 2] = 0  # value_len = 0 in run 10: no room for a handle
    off, ln, n, status = kvsep.sst_index_walk(bytes(hurt))
    assert (n, status) == (10, kvsep.SST_BAD_HANDLE)
    assert list(zip(off.tolist(), ln.tolist())) == handles[:10]
    hurt = bytearray(block)
    hurt[ro + 4 * 7:ro + 4 * 7 + 4] = restart(6).to_bytes(4, "little")  # restart[7] not above restart[6]
    off, ln, n, status = kvsep.sst_index_walk(bytes(hurt))
    assert status == kvsep.SST_BAD_RESTARTS and n >= 7 and list(zip(off.tolist(), ln.tolist()))[:7] == handles[:7]
    for short in (b"", b"\x00\x00\x00", (5).to_bytes(4, "little"), bytes(block[:-4]) + (10 ** 6).to_bytes(4, "little")):
        assert kvsep.sst_index_walk(short)[2:] == (0, kvsep.SST_BAD_RESTARTS)
    assert kvsep.sst_index_walk((0).to_bytes(4, "little"))[2:] == (0, kvsep.SST_OK)  # no restart: empty and valid


def test_bad_footers(golden_table):
    img, _ = golden_table
    bad = ((0, 0, 0, 0), kvsep.SST_BAD_FOOTER)
    assert kvsep.sst_footer(img[-47:]) == bad
    assert kvsep.sst_footer(b"") == bad
    wrong = bytearray(img)
    wrong[-1] ^= 1
    assert kvsep.sst_footer(bytes(wrong)) == bad
    assert kvsep.sst_footer(img[1000:]) == bad  # the handles now leave the image
    assert kvsep.sst_footer(bytes([0x80]) * 40 + img[-8:]) == bad  # a varint that leaves the 40 bytes
    ok = T.footer((0, 43), (0, 43))  # off + len + 5 = n exactly
    assert kvsep.sst_footer(ok) == ((0, 43, 0, 43), kvsep.SST_OK)
    assert kvsep.sst_footer(T.footer((0, 44), (0, 43))) == bad
    assert kvsep.sst_footer(T.footer((2 ** 64 - 3, 10), (0, 43))[-48:]) == bad  # a sum past 2^64


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_bound_and_in_the_header(name):
    assert hasattr(kvsep.lib(), name)
    res, args = kvsep._SIGS[name]
    assert res is ctypes.c_int and len(args) == NARGS[name]
    assert name in kvsep.header_functions()


def test_abi_version_stays_and_the_codes_are_defined():
    assert kvsep.lib().kvsep_abi_version() == 4
    header = open(kvsep.HEADER_PATH).read()
    assert "#define KVSEP_ABI_VERSION 4" in header
    for k, name in enumerate(("OK", "BAD_FOOTER", "INDEX_CHECKSUM", "INDEX_COMPRESSED", "BAD_RESTARTS", "BAD_ENTRY",
                              "BAD_HANDLE", "CAP")):
        assert f"#define KVSEP_SST_{name} {k}" in header and getattr(kvsep, "SST_" + name) == k
    for m in ("sst_index_device", "sst_table_verify_device"):
        assert callable(getattr(kvsep.Context, m))


def test_refusals_come_before_the_context_or_a_device_is_touched():
    """Every refusal below is made with a context pointer that must not be dereferenced (null, or an address that
    holds no context): KVSEP_EINVAL comes back, with its reason."""
    L = kvsep.lib()
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    err = lambda: L.kvsep_last_error().decode()
    for ctx in (None, ctypes.c_void_p(8)):
        assert L.kvsep_sst_index_device(ctx, None, None, 64, p, p, p, 4, p, p) == -1 and "file_base" in err()
        assert L.kvsep_sst_index_device(ctx, None, p, 64, p, None, p, 4, p, p) == -1 and "off or len" in err()
        assert L.kvsep_sst_index_device(ctx, None, p, 64, p, p, p, 4, None, p) == -1 and "nblocks or status" in err()
        assert L.kvsep_sst_index_device(ctx, None, p, 64, p, p, p, 4, p, None) == -1 and "nblocks or status" in err()
        assert L.kvsep_sst_index_device(ctx, None, p, 64, p, p, p, 2 ** 32, p, p) == -1 and "cap over" in err()
        assert L.kvsep_sst_index_device(ctx, None, p, 64, None, p, p, 4, p, p) == -1 and "null handle" in err()
        table = lambda *a: L.kvsep_sst_table_verify_device(ctx, None, *a)
        for cap in (0, 1):
            assert table(p, 64, p, p, p, p, p, p, 4, p, cap, 0, p, p, p) == -1 and "cap below 2" in err()
        assert table(None, 64, p, p, p, p, p, p, 4, p, 4, 0, p, p, p) == -1 and "file_base" in err()
        assert table(p, 64, None, p, p, p, p, p, 4, p, 4, 0, p, p, p) == -1 and "off or len" in err()
        assert table(p, 64, p, None, p, p, p, p, 4, p, 4, 0, p, p, p) == -1 and "off or len" in err()
        assert table(p, 64, p, p, None, p, p, p, 4, p, 4, 0, p, p, p) == -1 and "crc or handles" in err()
        assert table(p, 64, p, p, p, p, p, None, 4, p, 4, 0, p, p, p) == -1 and "bad_idx" in err()
        assert table(p, 64, p, p, p, p, p, p, 4, p, 4, 0, None, p, p) == -1 and "nblocks or status" in err()
        assert table(p, 64, p, p, p, p, p, p, 4, p, 4, 0, p, None, p) == -1 and "crc or handles" in err()
        assert table(p, 64, p, p, p, p, p, p, 4, p, 4, 0, p, p, None) == -1 and "nblocks or status" in err()
    assert L.kvsep_sst_index_device(None, None, p, 64, p, p, p, 4, p, p) == -1 and "null ctx" in err()
    assert L.kvsep_sst_table_verify_device(None, None, p, 64, p, p, p, p, p, p, 4, p, 4, 0, p, p, p) == -1
    assert "null ctx" in err()
    assert L.kvsep_sst_footer(p, 64, None, p) == -1 and L.kvsep_sst_footer(None, 64, p, p) == -1
    assert L.kvsep_sst_index_walk(p, 8, None, p, 1, p, p) == -1 and L.kvsep_sst_index_walk(p, 8, p, p, 1, None, p) == -1
