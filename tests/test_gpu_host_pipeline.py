"""The host staging pipeline (csrc/crc32c_host.cpp, grouping rules in csrc/host_slots.h) at its real limits: 64 MiB slots
and 65,536 blocks per slot job.  Every host-memory entry point goes through the span loop, the gather loop and the
segment chain of a long block; here each runs at and one past both limits, with long blocks that arrive on either slot
parity behind 0, 1 and 2 unretired jobs, with offsets in any order, and through the framings, the drop-in Extend and a
2-member group.  Every result is compared bit for bit with the oracle.  Needs a gfx950 device (`-m gpu`).

One module-scoped buffer of ~200 MiB (pageable and pinned copies of the same bytes) carries every case; the CRCs of the
few long ranges are computed by the oracle once and shared."""
import ctypes

import numpy as np
import pytest

import framing_builders as FB
import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
MiB = 1 << 20
SLOT = 64 * MiB   # host_slots.h kSlotBytes
CAP = 1 << 16     # host_slots.h kSlotBlocks
N = 200 * MiB     # the shared buffer
SENTINEL = 0xDEADBEEF
KVSEP_EINVAL = -1
VP = ctypes.c_void_p
LONG_OFF, LONG_INIT = 3, 0x9E3779B9  # every long block starts here (an odd offset) with this init
MEMS = ["pageable", "pinned"]


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    """{"pageable": array, "pinned": array}: the same N splitmix64 bytes twice."""
    d = torch.empty(N, dtype=torch.uint8, device=DEV)
    kvsep.fill_splitmix64(d.data_ptr(), N, 20261020, 0)
    pinned = torch.empty(N, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(d)
    torch.cuda.synchronize()
    pageable = d.cpu().numpy()
    del d
    assert np.array_equal(pageable[:4096], splitmix64_bytes(4096, 20261020, 0))
    yield {"pageable": pageable, "pinned": pinned.numpy(), "_keep": pinned}


class Ref:
    """The oracle over the shared buffer; blocks of 1 MiB and more are computed once per (off, len, init)."""

    def __init__(self, oracle, buf):
        self.oracle, self.buf, self.big = oracle, buf, {}

    def __call__(self, off, ln, init=None):
        off = np.asarray(off, np.uint64)
        ln = np.asarray(ln, np.uint64)
        ini = np.zeros(off.size, np.uint32) if init is None else np.asarray(init, np.uint32)
        out = np.zeros(off.size, np.uint32)
        small = ln < MiB
        if small.any():
            out[small] = self.oracle.batch(self.buf, off[small], ln[small], ini[small], threads=8)
        todo = [k for k in np.flatnonzero(~small) if (int(off[k]), int(ln[k]), int(ini[k])) not in self.big]
        if todo:
            got = self.oracle.batch(self.buf, off[todo], ln[todo], ini[todo], threads=16)
            for k, v in zip(todo, got):
                self.big[(int(off[k]), int(ln[k]), int(ini[k]))] = v
        for k in np.flatnonzero(~small):
            out[k] = self.big[(int(off[k]), int(ln[k]), int(ini[k]))]
        return out


@pytest.fixture(scope="module")
def ref(oracle, host):
    return Ref(oracle, host["pageable"])


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def span_raw(ctx, base_addr, span_bytes, off, ln, init, out):
    """kvsep_crc32c_batch_host_span as called: returns rc, results land in `out` (prefilled by the caller)."""
    off, ln = u64(off), u64(ln)
    ip = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    return kvsep.lib().kvsep_crc32c_batch_host_span(
        ctx._h, VP(base_addr), span_bytes, off.ctypes.data_as(VP), ln.ctypes.data_as(VP),
        None if ip is None else ip.ctypes.data_as(VP), out.ctypes.data_as(VP) if out.size else None, off.size)


def span(ctx, arr, off, ln, init=None):
    out = np.full(len(off), SENTINEL, np.uint32)
    assert span_raw(ctx, arr.ctypes.data, arr.nbytes, off, ln, init, out) == 0, kvsep.lib().kvsep_last_error()
    return out


def gather(ctx, arr, off, ln, init=None):
    """kvsep_crc32c_batch_host with block i's pointer at arr + off[i] (no per-block Python object)."""
    off, ln = u64(off), u64(ln)
    ptr = u64(off + np.uint64(arr.ctypes.data))
    ip = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    out = np.full(off.size, SENTINEL, np.uint32)
    rc = kvsep.lib().kvsep_crc32c_batch_host(ctx._h, None if ip is None else ip.ctypes.data_as(VP),
                                             ptr.ctypes.data_as(VP), ln.ctypes.data_as(VP), out.ctypes.data_as(VP),
                                             off.size)
    assert rc == 0, kvsep.lib().kvsep_last_error()
    return out


def tiny_blocks(count, seed, window=4 * MiB, base=0, maxlen=40):
    """count blocks of 0 .. maxlen bytes at random offsets of a window, with random inits."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, maxlen + 1, count).astype(np.uint64)
    off = (rng.integers(0, window - maxlen, count) + base).astype(np.uint64)
    init = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    return off, ln, init


def check(got, exp, what):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} of {exp.size} blocks differ, first at index {bad[0]} " \
                          f"(got {got[bad[0]]:#x}, oracle {exp[bad[0]]:#x})"


# ------------------------------------------------------------------ the block-count cap
@pytest.mark.parametrize("count", [CAP - 1, CAP, CAP + 1, 2 * CAP, 2 * CAP + 1])
def test_span_block_count_cap(ctx, host, ref, count):
    off, ln, init = tiny_blocks(count, count)
    ln[[0, -1]] = [33, 40]  # the blocks next to either end are real
    exp_init, exp_plain = ref(off, ln, init), ref(off, ln)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp_init, f"{mem}, {count} blocks with init")
        check(span(ctx, host[mem], off, ln), exp_plain, f"{mem}, {count} blocks without init")


@pytest.mark.parametrize("count", [CAP + 1, 2 * CAP + 1])
def test_gather_block_count_cap_bytes_objects(ctx, host, ref, count):
    off, ln, init = tiny_blocks(count, 7 + count)
    ln[::9] = 0  # some of them empty
    ln[[CAP - 1, CAP, -1]] = [17, 31, 40]
    buf = host["pageable"]
    blocks = [buf[o:o + l].tobytes() for o, l in zip(off.tolist(), ln.tolist())]
    check(ctx.batch_host(blocks, init), ref(off, ln, init), f"{count} bytes objects with init")
    check(ctx.batch_host(blocks), ref(off, ln), f"{count} bytes objects without init")


# ------------------------------------------------------------------ the byte cap
def with_tail(off, ln, seed):
    """The given blocks followed by 50 tiny ones (they land in the group after the edge, or share it)."""
    toff, tln, _ = tiny_blocks(50, seed, base=100 * MiB)
    off, ln = np.concatenate([u64(off), toff]), np.concatenate([u64(ln), tln])
    init = np.random.default_rng(seed).integers(0, 2**32, off.size, dtype=np.uint64).astype(np.uint32)
    return off, ln, init


@pytest.mark.parametrize("case", ["range_exact", "range_plus_1", "130x1MiB_shifted", "block_exact_alone",
                                  "block_exact_between"])
def test_span_byte_cap(ctx, host, ref, case):
    if case == "range_exact":      # two adjacent blocks whose covering range is exactly one slot
        off, ln = [5, 5 + SLOT - 4096], [SLOT - 4096, 4096]
    elif case == "range_plus_1":   # ... and one byte over: the second block opens a new group
        off, ln = [5, 5 + SLOT - 4096], [SLOT - 4096, 4097]
    elif case == "130x1MiB_shifted":
        off, ln = 1 + MiB * np.arange(130), np.full(130, MiB)
    elif case == "block_exact_alone":  # exactly a slot: a group of its own, not the segment chain
        off, ln = [7], [SLOT]
    else:
        off, ln = [100, 7, 9 + SLOT, 64], [30, SLOT, 25, 0]
    if case == "block_exact_alone":
        off, ln, init = u64(off), u64(ln), np.array([0x80000001], np.uint32)
    else:
        off, ln, init = with_tail(off, ln, 11)
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, f"{case}, {mem}")


@pytest.mark.parametrize("blk", [16 * MiB - 1, 16 * MiB + 1])
def test_gather_byte_cap(ctx, host, ref, blk):
    # 16 MiB - 1: four blocks round up to 16 MiB starts and fill one slot exactly; 16 MiB + 1: the fourth spills over
    off, ln, init = with_tail(3 + 17 * MiB * np.arange(4), [blk] * 4, blk)
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(gather(ctx, host[mem], off, ln, init), exp, f"4 x {blk} B, {mem}")
    check(gather(ctx, host["pageable"], off[:4], ln[:4]), ref(off[:4], ln[:4]), f"4 x {blk} B alone")


# ------------------------------------------------------------------ long blocks: the segment chain
LONGS = [SLOT + 1, 2 * SLOT, 2 * SLOT + 1, 3 * SLOT + 1]  # 2, 2, 3 and 4 segments


def around_long(longs, before, after, seed):
    """`before` tiny blocks, the long blocks (each at LONG_OFF with LONG_INIT), `after` tiny blocks."""
    boff, bln, binit = tiny_blocks(before, seed)
    aoff, aln, ainit = tiny_blocks(after, seed + 1, base=150 * MiB)
    if before:
        bln[[0, -1]] = [40, 39]
    if after:
        aln[[0, -1]] = [38, 37]
    k = len(longs)
    return (np.concatenate([boff, u64([LONG_OFF] * k), aoff]), np.concatenate([bln, u64(longs), aln]),
            np.concatenate([binit, np.full(k, LONG_INIT, np.uint32), ainit]))


# before -> the jobs in flight when the long block arrives: none; one group (the long block's own turn would be
# slot 1); two groups (65,536 + 4 blocks: both slots busy, slot 0 again)
PLACEMENTS = {"first": (0, 20), "last": (20, 0), "after_one_group": (20, 20), "after_two_groups": (CAP + 4, 20)}


@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("n", LONGS)
def test_long_block_placements(ctx, host, ref, n, place):
    before, after = PLACEMENTS[place]
    off, ln, init = around_long([n], before, after, n % 1000 + before)
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, f"span, {mem}, {n} B {place}")
        check(gather(ctx, host[mem], off, ln, init), exp, f"gather, {mem}, {n} B {place}")


def test_two_long_blocks_back_to_back(ctx, host, ref):
    off, ln, init = around_long([SLOT + 1, 2 * SLOT + 1], 20, 20, 5)
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, f"span, {mem}")
        check(gather(ctx, host[mem], off, ln, init), exp, f"gather, {mem}")
    off, ln, init = around_long([2 * SLOT, SLOT + 1], 0, 0, 6)  # nothing around them
    check(span(ctx, host["pinned"], off, ln, init), ref(off, ln, init), "span, two long blocks alone")


# ------------------------------------------------------------------ order and overlap (span form)
def packed_layout(count, seed):
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, 60_000, count).astype(np.uint64)
    off = np.zeros(count, np.uint64)
    off[1:] = np.cumsum(ln[:-1] + np.uint64(3), dtype=np.uint64)  # 3-byte gaps: odd alignments
    init = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    return off + np.uint64(11), ln, init


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_span_offsets_in_any_order(ctx, host, ref, order):
    # ~90 MiB of packed blocks: more than one group, and lo moves down inside each of them
    off, ln, init = packed_layout(3000, 31)
    assert int(off[-1] + ln[-1]) > SLOT
    idx = np.arange(3000)[::-1] if order == "descending" else np.random.default_rng(32).permutation(3000)
    off, ln, init = off[idx], ln[idx], init[idx]
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, f"{order}, {mem}")


def test_span_heavy_overlap_understated_payload(ctx, host, ref):
    # 1,000 blocks of 1 MiB inside a 2 MiB window: one group whose staged range (the byte hint) is 2 MiB for 1000 MiB
    # of work
    k = np.arange(1000, dtype=np.uint64)
    off = np.uint64(50 * MiB + 1) + (k * np.uint64(4099)) % np.uint64(MiB)
    ln = np.full(1000, MiB, np.uint64)
    init = (k * np.uint64(2654435761) % np.uint64(2**32)).astype(np.uint32)
    exp = ref(off, ln, init)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, mem)


def test_span_zero_length_blocks_at_the_ends(ctx, host, ref):
    off = [0, N, 17, N, 5 * MiB, 0, N - 1, 70 * MiB, N]
    ln = [0, 0, 100, 0, 0, 64, 1, 4097, 0]
    init = np.arange(1, 10, dtype=np.uint32) * np.uint32(0x01010101)
    exp = ref(off, ln, init)
    assert [int(exp[i]) for i in (0, 1, 3, 4, 8)] == [int(init[i]) for i in (0, 1, 3, 4, 8)]  # Extend(init, "", 0)
    for mem in MEMS:
        check(span(ctx, host[mem], off, ln, init), exp, mem)
        check(span(ctx, host[mem], off, ln), ref(off, ln), mem + " without init")


def test_span_empty_calls(ctx, host):
    out = np.full(4, SENTINEL, np.uint32)
    assert span_raw(ctx, host["pageable"].ctypes.data, N, [], [], None, out[:0]) == 0  # count == 0
    assert span_raw(ctx, 0, 0, [], [], None, out[:0]) == 0
    assert (out == SENTINEL).all()
    init = np.array([0, 1, 0xFFFFFFFF, 0x12345678], np.uint32)
    assert span_raw(ctx, 0, 0, [0] * 4, [0] * 4, init, out) == 0  # span_bytes == 0, null base, only empty blocks
    assert np.array_equal(out, init)
    assert span_raw(ctx, 0, 0, [0] * 4, [0] * 4, None, out) == 0
    assert (out == 0).all()


@pytest.mark.parametrize("bad", ["off_past_span", "off_wraps", "len_over_span"])
def test_span_rejects_blocks_outside_the_span(ctx, host, bad):
    span_bytes = 1 * MiB
    off, ln = [10, 20, 30], [5, 6, 7]
    if bad == "off_past_span":
        off[1], ln[1] = span_bytes + 1, 0
    elif bad == "off_wraps":
        off[1], ln[1] = 2**64 - 1, 2
    else:
        off[1], ln[1] = 0, span_bytes + 1
    out = np.full(3, SENTINEL, np.uint32)
    for mem in MEMS:
        assert span_raw(ctx, host[mem].ctypes.data, span_bytes, off, ln, None, out) == KVSEP_EINVAL
        assert (out == SENTINEL).all()
    assert b"outside span" in kvsep.lib().kvsep_last_error()


# ------------------------------------------------------------------ framings across a group boundary
def np_mask(crc):
    crc = crc.astype(np.uint64)
    return ((((crc >> np.uint64(15)) | (crc << np.uint64(17))) + np.uint64(kvsep.MASK_DELTA)) &
            np.uint64(0xFFFFFFFF)).astype(np.uint32)


def put_le32(img, at, words):
    for b in range(4):
        img[(at + np.uint64(b)).astype(np.int64)] = ((words.astype(np.uint64) >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)


@pytest.fixture(scope="module")
def vlog(oracle):
    """An image of 140,000 records of 1 .. 24 payload bytes (db/value_log_writer.cc:46-76) and its walk."""
    k = 140_000
    rng = np.random.default_rng(77)
    ln = rng.integers(1, 25, k).astype(np.uint64)
    hdr = np.zeros(k, np.uint64)
    hdr[1:] = np.cumsum(ln[:-1] + np.uint64(8), dtype=np.uint64)
    img = splitmix64_bytes(int(hdr[-1] + 8 + ln[-1]), 78, 0)
    off = hdr + np.uint64(8)
    put_le32(img, hdr + np.uint64(4), ln)
    put_le32(img, hdr, np_mask(oracle.batch(img, off, ln, threads=8)))
    return img, off, ln


@pytest.mark.parametrize("bad", [None, CAP - 1, CAP, 2 * CAP])
def test_vlog_verify_across_group_boundaries(ctx, oracle, vlog, bad):
    img, off, ln = vlog
    k = off.size
    assert kvsep.vlog_walk(img)[3] == img.size and np.array_equal(kvsep.vlog_walk(img)[0], off)
    if bad is None:
        assert ctx.vlog_verify(img, with_drop=True) == (k, k, img.size, 0)
        return
    img = img.copy()
    img[int(off[bad]) + int(ln[bad]) // 2] ^= 0x04
    stored = int.from_bytes(img[int(off[bad]) - 8:int(off[bad]) - 4].tobytes(), "little")
    assert kvsep.mask(oracle.extend(0, img[int(off[bad]):int(off[bad] + ln[bad])].tobytes())) != stored
    # the reader keeps the records before the first mismatch and reports that record's payload as dropped
    assert ctx.vlog_verify(img, with_drop=True) == (k, bad, int(off[bad - 1] + ln[bad - 1]), int(ln[bad]))


def test_log_frame_and_verify_across_a_group_boundary(ctx, oracle):
    k = 70_000
    data = splitmix64_bytes(10 * k, 79, 0).tobytes()
    records = [data[10 * i:10 * i + 10] for i in range(k)]
    want, phys = FB.log_image(records, oracle)
    assert len(phys) > CAP  # the tee gather runs over more than one slot job
    got = ctx.log_frame(records)
    assert got == want
    ok = ctx.log_verify(got)
    assert ok.size == len(phys) and ok.all()


def test_sst_host_forms_across_a_group_boundary(ctx, oracle):
    # test_sst_host_forms_large_batch_match_oracle has 20,000 blocks: below the cap, so this case is needed
    k = 70_000
    rng = np.random.default_rng(80)
    ln = rng.integers(1, 30, k)
    data = splitmix64_bytes(int(ln.sum()), 81, 0).tobytes()
    ends = np.cumsum(ln)
    blocks = [data[e - l:e] for e, l in zip(ends.tolist(), ln.tolist())]
    types = rng.integers(0, 2, k).astype(np.uint8)
    img, offs, words = FB.sst_image(blocks, types.tolist(), oracle)
    assert np.array_equal(ctx.sst_trailers(blocks, types), words)
    lens = ln.astype(np.uint64)
    out, fb, nb = ctx.sst_verify(img, offs, lens)
    assert (fb, nb) == (-1, 0)
    for i in (0, CAP - 1, CAP, k - 1):  # Value(block, len + 1) itself
        assert int(out[i]) == oracle.extend(0, img[int(offs[i]):int(offs[i] + lens[i]) + 1])
    bad = [CAP - 1, CAP, k - 1]
    img = bytearray(img)
    for i in bad:
        img[int(offs[i])] ^= 0x40
    out, fb, nb = ctx.sst_verify(bytes(img), offs, lens)
    assert (fb, nb) == (bad[0], len(bad))


# ------------------------------------------------------------------ the drop-in Extend at its default threshold
def offload_stats():
    v = [ctypes.c_uint64(0) for _ in range(3)]
    kvsep.lib().kvsep_offload_stats(*[ctypes.byref(x) for x in v])
    return [x.value for x in v]


def test_dropin_extend_at_the_default_threshold(oracle, host):
    buf = host["pageable"]
    sizes = [SLOT - 1, SLOT, SLOT + 1, 2 * SLOT + 1]
    exp = [oracle.extend_addr(LONG_INIT, buf.ctypes.data + 3, n) for n in sizes]
    kvsep.lib().kvsep_set_offload_wait(1)  # queue for the GPU leg instead of diverting to the host leg
    gpu0, host0, fail0 = offload_stats()
    try:
        got = [kvsep.extend(LONG_INIT, buf[3:3 + n]) for n in sizes]
    finally:
        kvsep.lib().kvsep_set_offload_wait(0)
    gpu1, host1, fail1 = offload_stats()
    assert got == exp
    # 64 MiB - 1 is below the threshold (host leg, not counted); the other three ran on the GPU
    assert (gpu1 - gpu0, host1 - host0, fail1 - fail0) == (3, 0, 0)


# ------------------------------------------------------------------ a 2-member group
def test_group_host_span_with_a_long_block_at_the_cut(host, ref):
    g = kvsep.Group([0, 0] if kvsep.device_count() < 2 else [0, 1])
    try:
        off, ln, init = around_long([SLOT + 1], 70_000, 70_000, 90)
        at = 70_000
        bounds = kvsep.partition(ln, 2)
        assert int(bounds[1]) in (at, at + 1)  # the byte-balanced cut falls at the long block
        exp = ref(off, ln, init)
        for mem in MEMS:
            check(g.batch_host_span(host[mem], off, ln, init=init), exp, f"group batch, {mem}")
        stored = np_mask(exp)
        out, fb, nb = g.batch_host_span(host["pageable"], off, ln, init=init, expected_masked=stored)
        check(out, exp, "group verify, clean")
        assert (fb, nb) == (2**64 - 1, 0)
        plant = [CAP + 5, at - 1, at, at + 1, 2 * CAP + 9, off.size - 1]  # both members' parts, and the long block
        assert plant[0] < int(bounds[1]) <= plant[3]
        stored[plant] ^= np.uint32(0x10)
        out, fb, nb = g.batch_host_span(host["pinned"], off, ln, init=init, expected_masked=stored)
        check(out, exp, "group verify, planted")
        assert (fb, nb) == (plant[0], len(plant))
    finally:
        g.close()
