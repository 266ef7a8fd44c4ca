"""The SST table writer's host forms against the reference's own file: kvsep_sst_index_keys gives the keys and handles
of tests/golden/ref_table.sst's index block as sst_tables.parse_index reads them; kvsep_sst_index_build with those, and
kvsep_sst_footer_build, reproduce the file's index block, metaindex block, both trailers and footer byte for byte; the
same holds against sst_tables.index_block / footer for synthetic tables and keep masks.  The refusals and the argument
checks need no device.  None of these symbols exists before the table writer."""
import ctypes
import os

import numpy as np
import pytest

import kvsep
import sst_tables as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1  # KVSEP_EINVAL
NARGS = {"kvsep_sst_index_keys": 9, "kvsep_sst_index_keys_device": 12, "kvsep_sst_index_build": 12,
         "kvsep_sst_footer_build": 5, "kvsep_sst_index_build_device": 14, "kvsep_sst_table_finish_device": 15,
         "kvsep_sst_table_rewrite_device": 22}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ref_table.sst"), "rb") as f:
        img = f.read()
    handles, status = kvsep.sst_footer(img)
    assert status == kvsep.SST_OK
    return img, handles


def keys_of(block, key_off, key_len):
    return [bytes(block[int(o):int(o) + int(k)]) for o, k in zip(key_off, key_len)]


def test_precondition_of_the_identity_rewrite(golden):
    """What the GPU identity test rests on: data blocks back to back from 0, the 8-byte metaindex block right after.
    (A check of the fixture, through entry points that predate the table writer: it passes without the feature; every
    other test of this file needs the new symbols.)"""
    img, (moff, mlen, ioff, ilen) = golden
    off, ln, nblocks, status = kvsep.sst_index_walk(img[ioff:ioff + ilen])
    assert status == kvsep.SST_OK and nblocks == 52
    p = 0
    for o, k in zip(off.tolist(), ln.tolist()):
        assert o == p
        p = o + k + 5
    assert (moff, mlen) == (p, 8) and ioff == moff + 13 and len(img) == ioff + ilen + 5 + 48


def test_keys_walk_of_the_reference_table(golden):
    img, (_, _, ioff, ilen) = golden
    block = img[ioff:ioff + ilen]
    keys, handles = T.parse_index(block)
    off, ln, ko, kl, nblocks, status = kvsep.sst_index_keys(block)
    assert (nblocks, status) == (52, kvsep.SST_OK)
    assert list(zip(off.tolist(), ln.tolist())) == handles
    assert keys_of(block, ko, kl) == keys
    o2, l2, _, _ = kvsep.sst_index_walk(block)
    assert (off == o2).all() and (ln == l2).all()


@pytest.mark.parametrize("cap", [0, 1, 51, 52, 60])
def test_keys_walk_cap(golden, cap):
    img, (_, _, ioff, ilen) = golden
    block = img[ioff:ioff + ilen]
    keys, handles = T.parse_index(block)
    off, ln, ko, kl, nblocks, status = kvsep.sst_index_keys(block, cap=cap)
    m = min(cap, 52)
    assert (nblocks, status, off.size) == (52, kvsep.SST_OK, cap)
    assert keys_of(block, ko[:m], kl[:m]) == keys[:m]
    assert not ko[m:].any() and not kl[m:].any() and not off[m:].any() and not ln[m:].any()


def test_build_reproduces_the_reference_file(golden):
    img, (moff, mlen, ioff, ilen) = golden
    block = img[ioff:ioff + ilen]
    off, ln, ko, kl, _, _ = kvsep.sst_index_keys(block)
    out, out_len, status = kvsep.sst_index_build(block, ko, kl, off, ln)
    assert (status, out_len) == (kvsep.SSTW_OK, ilen)
    assert out == img[ioff:ioff + ilen + 5], "index block and its trailer"
    meta, meta_len, status = kvsep.sst_index_build(b"", [], [], [], [])
    assert (status, meta_len) == (kvsep.SSTW_OK, 8)
    assert meta == img[moff:moff + 13], "metaindex block and its trailer"
    assert kvsep.sst_footer_build((moff, mlen), (ioff, ilen)) == img[-48:]
    # the whole tail of the file, in place at its position
    dst = np.zeros(len(img), np.uint8)
    kvsep.sst_index_build(b"", [], [], [], [], dst=dst, at=moff)
    _, n, _ = kvsep.sst_index_build(block, ko, kl, off, ln, dst=dst, at=moff + 13)
    dst[moff + 13 + n + 5:] = np.frombuffer(kvsep.sst_footer_build((moff, 8), (moff + 13, n)), np.uint8)
    assert dst[moff:].tobytes() == img[moff:] and not dst[:moff].any()


MASKS = {
    "none": lambda n: np.zeros(n, np.uint8),
    "all": lambda n: np.ones(n, np.uint8),
    "alternating": lambda n: (np.arange(n) % 2).astype(np.uint8),
    "first": lambda n: (np.arange(n) == 0).astype(np.uint8),
    "last": lambda n: (np.arange(n) == n - 1).astype(np.uint8),
}


@pytest.mark.parametrize("nblocks", [0, 1, 64, 65, 1025])
@pytest.mark.parametrize("mask", list(MASKS))
def test_build_of_synthetic_tables(nblocks, mask):
    img, off, ln, meta, index = T.build_table(nblocks)
    block = img[index[0]:index[0] + index[1]].tobytes()
    o, l, ko, kl, nb, status = kvsep.sst_index_keys(block)
    assert (nb, status) == (nblocks, kvsep.SST_OK) and (o == off).all() and (l == ln).all()
    keys = keys_of(block, ko, kl)
    assert keys == [T.key_of(i) for i in range(nblocks)]
    keep = MASKS[mask](nblocks)
    new_off = np.arange(nblocks, dtype=np.uint64) * 1000003 + 7  # new handles, as a salvage would give
    if nblocks > 2:
        new_off[nblocks // 2] = kvsep.OFFSET_SKIP  # a block that was not laid out, whatever keep says
    kept = [i for i in range(nblocks) if keep[i] and int(new_off[i]) != kvsep.OFFSET_SKIP]
    want = T.index_block([keys[i] for i in kept], [(int(new_off[i]), int(ln[i])) for i in kept])
    out, out_len, status = kvsep.sst_index_build(block, ko, kl, new_off, ln, keep=keep)
    assert (status, out_len) == (kvsep.SSTW_OK, len(want))
    assert out == want + T.trailer(want)
    if mask == "all" and nblocks <= 2:
        assert kvsep.sst_index_build(block, ko, kl, off, ln, keep=None)[0] == block + T.trailer(block)
    assert kvsep.sst_footer_build(meta, index) == T.footer(meta, index)


def test_handle_and_key_widths():
    """Handle values on both sides of every varint width, key lengths on both sides of the two-byte non_shared."""
    vals = [0, 1]
    for b in range(7, 64, 7):
        vals += [(1 << b) - 1, 1 << b]
    vals += [(1 << 64) - 2]  # 2^64 - 1 is OFFSET_SKIP
    klens = [0, 1, 127, 128, 4097, 16384]
    src = kvsep.splitmix64_bytes(sum(klens) + 16, 9).tobytes()
    keys, ko, kl, handles = [], [], [], []
    p = 3
    for i, v in enumerate(vals):
        k = klens[i % len(klens)]
        ko.append(p), kl.append(k), keys.append(src[p:p + k])
        p = (p + k) % (len(src) - 16384)
        handles.append((v, vals[-1 - i]))
    want = T.index_block(keys, handles)
    out, out_len, status = kvsep.sst_index_build(src, ko, kl, [h[0] for h in handles], [h[1] for h in handles])
    assert (status, out_len) == (kvsep.SSTW_OK, len(want)) and out == want + T.trailer(want)
    for m, i in ((vals[3], vals[-1]), (vals[-1], vals[2])):
        assert kvsep.sst_footer_build((m, i), (i, m)) == T.footer((m, i), (i, m))


def test_interval_two_stops_at_its_second_entry():
    keys = [T.key_of(i) for i in range(6)]
    handles = [(100 * i, 50 + i) for i in range(6)]
    block = T.index_block(keys, handles, 2)
    off, ln, ko, kl, nblocks, status = kvsep.sst_index_keys(block, cap=6)
    assert (nblocks, status) == (1, kvsep.SST_SHARED_KEY)
    assert (int(off[0]), int(ln[0])) == handles[0] and keys_of(block, ko[:1], kl[:1]) == keys[:1]
    assert not off[1:].any() and not kl[1:].any()
    assert kvsep.sst_index_walk(block)[2:] == (6, kvsep.SST_OK)  # the plain walk is unchanged
    # keys that share nothing are whole at any interval
    apart = [bytes([65 + i]) * 5 for i in range(6)]
    block = T.index_block(apart, handles, 2)
    off, ln, ko, kl, nblocks, status = kvsep.sst_index_keys(block)
    assert (nblocks, status) == (6, kvsep.SST_OK) and keys_of(block, ko, kl) == apart


def test_no_room_and_too_large():
    keys = [T.key_of(i) for i in range(3)]
    src = b"".join(keys)
    kl = [len(k) for k in keys]
    ko = [0, kl[0], kl[0] + kl[1]]
    want = T.index_block(keys, [(1, 2), (3, 4), (5, 6)])
    for at in (0, 5):
        dst = np.full(at + len(want) + 5, 0xEE, np.uint8)
        _, out_len, status = kvsep.sst_index_build(src, ko, kl, [1, 3, 5], [2, 4, 6], dst=dst, at=at)
        assert (status, out_len) == (kvsep.SSTW_OK, len(want)) and dst[at:].tobytes() == want + T.trailer(want)
        assert (dst[:at] == 0xEE).all()
        short = np.full(at + len(want) + 4, 0xEE, np.uint8)
        _, out_len, status = kvsep.sst_index_build(src, ko, kl, [1, 3, 5], [2, 4, 6], dst=short, at=at)
        assert (status, out_len) == (kvsep.SSTW_NO_ROOM, len(want)) and (short == 0xEE).all()
    dst = np.full(64, 0xEE, np.uint8)
    for at in (65, (1 << 64) - 1, (1 << 64) - 40):  # past the end, and sums that would wrap
        _, out_len, status = kvsep.sst_index_build(src, ko, kl, [1, 3, 5], [2, 4, 6], dst=dst, at=at)
        assert (status, out_len) == (kvsep.SSTW_NO_ROOM, len(want)) and (dst == 0xEE).all()
    # a key_len a varint32 cannot hold: too large, decided before a key byte is read
    _, out_len, status = kvsep.sst_index_build(src, [0], [1 << 32], [1], [2], dst=dst, at=0)
    assert (status, out_len) == (kvsep.SSTW_TOO_LARGE, 0) and (dst == 0xEE).all()


def test_symbols_are_declared_exported_and_bound():
    lib = kvsep.lib()
    declared = kvsep.header_functions()
    for name, nargs in NARGS.items():
        assert name in declared
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.kvsep_abi_version() == 4
    assert (kvsep.SST_SHARED_KEY, kvsep.SSTW_OK, kvsep.SSTW_TOO_LARGE, kvsep.SSTW_NO_ROOM, kvsep.SSTW_SOURCE) == \
        (8, 0, 1, 2, 3)


def test_device_forms_refuse_bad_arguments_without_a_device():
    lib = kvsep.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below is refused first
    null = ctypes.c_void_p(0)
    rc = lib.kvsep_sst_index_keys_device(null, null, one, 64, one, one, one, null, one, 4, one, one)
    assert rc == EINVAL and b"key_off" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_index_keys_device(null, null, one, 64, one, one, one, one, one, 4, one, one)
    assert rc == EINVAL and b"null ctx" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_index_build_device(null, null, one, null, one, one, one, null, 3, one, 64, one, one, one)
    assert rc == EINVAL and b"null key or handle array" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_index_build_device(null, null, one, one, one, one, one, null, 3, one, 64, null, one, one)
    assert rc == EINVAL and b"position" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_index_build_device(null, null, one, one, one, one, one, null, 1 << 32, one, 64, one, one, one)
    assert rc == EINVAL and b"2^32 - 1" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_index_build_device(null, null, one, one, one, one, one, null, 3, one, 64, one, one, one)
    assert rc == EINVAL and b"null ctx" in lib.kvsep_last_error()
    rc = lib.kvsep_sst_table_finish_device(null, null, one, one, one, one, one, null, 3, one, 64, one, one, null, one)
    assert rc == EINVAL and b"table_bytes" in lib.kvsep_last_error()
    args = [null, null, one, 64, one, 64] + [one] * 7 + [1, 0] + [one] * 7
    assert lib.kvsep_sst_table_rewrite_device(*args) == EINVAL and b"cap below 2" in lib.kvsep_last_error()
    args[13] = 4
    assert lib.kvsep_sst_table_rewrite_device(*args) == EINVAL and b"null ctx" in lib.kvsep_last_error()
    args[12] = null  # dst_off
    assert lib.kvsep_sst_table_rewrite_device(*args) == EINVAL and b"null argument" in lib.kvsep_last_error()
