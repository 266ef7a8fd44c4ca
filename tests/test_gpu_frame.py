"""GPU: the device write side -- kvsep_crc32c_pack_device (crc32c_pack_kernel) and the vlog / SST frame forms built on
it.  Every destination is a 0xA5-filled buffer with at least 256 canary bytes around the records (and canaries in
deliberate gaps), handed to the call whole, and the WHOLE buffer is compared with an image built by numpy.

  * alignment sweep: source alignment 0..15 x destination alignment 0..15 x 30 lengths in one batch, the records back to
    back in an order that gives every record its alignment (an Euler circuit over the alignments), block indices
    shuffled against the placement, so every edge is shared with a record another wave writes; then with 1-byte gaps;
  * runs of 0, 1, 2, 8, 65 and 300 segments, zero-length segments at the start, middle and end, segments out of order,
    overlapping and shared between blocks, first[] out of range (the documented clamp), nseg == 0, count == 0;
  * block lengths around the 64 KiB tile at odd alignments, and one block of 8 MiB + 13 alone in its batch;
  * dst_bytes one byte short of the last record: that record is not written at all;
  * vlog: the payloads of tests/golden/ref_small.vlog, each as three segments at odd cuts scattered over a shuffled
    source, reproduce the file byte for byte on every CRC route; a random batch equals the host form;
  * SST: the blocks of tests/golden/ref_table.sst, scattered, framed at their handles reproduce that part of the file on
    every CRC route, and the read check passes on the result;
  * a reserved vlog_frame_device call captured into a graph and replayed into a re-poisoned destination.
Needs a gfx950 device (`-m gpu`)."""
import json
import os
import re

import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY, MARGIN = 0xA5, 256
BIG = 2**64 - 1
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024,
           1025, 4095, 4096, 4097]


def tile_bytes():
    src = open(os.path.join(os.path.dirname(kvsep.LIB_PATH), "..", "csrc", "pack_run.h")).read()
    return int(re.search(r"constexpr uint64_t kTile = (\d+) \* 1024;", src).group(1)) * 1024


T = tile_bytes()


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


def runs_of(first, nseg):
    """The documented clamp: both ends to nseg, a run that ends before it starts is empty."""
    out = []
    for f0, f1 in zip(first[:-1], first[1:]):
        s, e = min(int(f0), nseg), min(int(f1), nseg)
        out.append((s, max(s, e)))
    return out


def image(src, seg_off, seg_len, runs, dst_off, size, dst_bytes, frame=None, crc=None, types=None):
    """The expected destination: canary everywhere but the framed blocks that lie inside [0, dst_bytes)."""
    img = np.full(size, CANARY, np.uint8)
    lead, trail = (8, 0) if frame == "vlog" else (0, 5) if frame == "sst" else (0, 0)
    for i, (s, e) in enumerate(runs):
        parts = [src[int(seg_off[j]):int(seg_off[j]) + int(seg_len[j])] for j in range(s, e)]
        body = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        p = int(dst_off[i])
        if p + lead + body.size + trail > dst_bytes:
            continue
        if frame == "vlog":
            head = np.array([kvsep.mask(int(crc[i])), body.size & 0xFFFFFFFF], "<u4").view(np.uint8)
            img[p:p + 8] = head
        img[p + lead:p + lead + body.size] = body
        if frame == "sst":
            q = p + body.size
            img[q] = types[i]
            img[q + 1:q + 5] = np.array([int(crc[i])], "<u4").view(np.uint8)
    return img


def pack(ctx, d_src, seg_off, seg_len, first, dst_off, size, dst_bytes=None):
    dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.pack_device(d_src.data_ptr(), u64(seg_off), u64(seg_len), u64(first), dst.data_ptr(),
                    size if dst_bytes is None else dst_bytes, u64(dst_off), count=len(first) - 1, nseg=len(seg_len))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def same(got, exp, what=""):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:8]}: got {got[bad[:8]]}, want {exp[bad[:8]]}"


# ---------------------------------------------------------------- alignment sweep
def euler_order(blocks, gap, rng):
    """An order of all blocks (sa, da, len) such that, laid back to back with `gap` bytes between them from an offset
    that is 0 mod 16, every block starts at its da: an Euler circuit of the graph whose nodes are the 16 alignments and
    whose edges are the blocks, da -> da + len + gap (every node has as many edges in as out: Hierholzer)."""
    out = {a: [] for a in range(16)}
    for idx in rng.permutation(len(blocks)):
        out[blocks[idx][1]].append(int(idx))
    stack, path = [(0, None)], []
    while stack:
        v, e = stack[-1]
        if out[v]:
            idx = out[v].pop()
            stack.append(((v + blocks[idx][2] + gap) % 16, idx))
        else:
            stack.pop()
            if e is not None:
                path.append(e)
    path.reverse()
    assert len(path) == len(blocks)
    return path


@pytest.fixture(scope="module")
def sweep_source():
    rng = np.random.default_rng(20261020)
    combos = [(sa, da, n) for sa in range(16) for da in range(16) for n in LENGTHS]
    blocks = [combos[i] for i in rng.permutation(len(combos))]  # block index order: shuffled
    slot, seg_off = 0, np.zeros(len(blocks), np.uint64)
    for i in rng.permutation(len(blocks)):  # and so is the source
        seg_off[i] = slot + blocks[i][0]
        slot += (blocks[i][2] + 15) // 16 * 16 + 32
    src = splitmix64_bytes(slot + 16, 77, 0)
    return blocks, seg_off, src, dev8(src)


@pytest.mark.parametrize("gap", [0, 1], ids=["back_to_back", "one_byte_gaps"])
def test_alignment_sweep(ctx, sweep_source, gap):
    blocks, seg_off, src, d_src = sweep_source
    rng = np.random.default_rng(5 + gap)
    order = euler_order(blocks, gap, rng)
    dst_off, p = np.zeros(len(blocks), np.uint64), MARGIN
    for idx in order:
        assert p % 16 == blocks[idx][1]
        dst_off[idx] = p
        p += blocks[idx][2] + gap
    assert {(int(seg_off[i]) % 16, int(dst_off[i]) % 16, b[2]) for i, b in enumerate(blocks)} == {
        (sa, da, n) for sa in range(16) for da in range(16) for n in LENGTHS}
    size = p + MARGIN
    seg_len = np.array([b[2] for b in blocks], np.uint64)
    first = np.arange(len(blocks) + 1, dtype=np.uint64)
    got = pack(ctx, d_src, seg_off, seg_len, first, dst_off, size)
    same(got, image(src, seg_off, seg_len, runs_of(first, len(blocks)), dst_off, size, size), f"gap {gap}")


# ---------------------------------------------------------------- runs
@pytest.fixture(scope="module")
def payload():
    host = splitmix64_bytes(4 << 20, 4242, 0)
    return host, dev8(host)


def test_runs_of_every_shape(ctx, payload):
    host, d = payload
    rng = np.random.default_rng(11)
    per_block = [0, 1, 2, 8, 65, 300, 0, 3, 64, 300, 65, 1]
    seg_len, first = [], [0]
    for n in per_block:
        ln = rng.integers(0, 900, n)
        if n >= 3:
            ln[[0, n // 2, n - 1]] = 0  # zero-length segments at the start, middle and end of the run
        seg_len += ln.tolist()
        first.append(len(seg_len))
    nseg = len(seg_len)
    seg_len = np.array(seg_len, np.uint64)
    seg_off = rng.integers(0, host.size - 900, nseg).astype(np.uint64)  # anywhere: out of order, overlapping
    seg_off[seg_len == 0] = BIG - 5  # a zero-length segment is never dereferenced, whatever its offset
    # blocks that share segments with earlier ones (first[] steps back: the block in between is empty by the clamp), and
    # first[] values out of range
    first += [5, 80, 2**40, 70, BIG, nseg - 3, nseg + 7]
    first = np.array(first, np.uint64)
    runs = runs_of(first, nseg)
    used = np.zeros(nseg, int)
    for s, e in runs:
        used[s:e] += 1
    assert used.max() >= 2 and (0, 0) in runs and runs[-1] == (nseg - 3, nseg)  # shared segments, clamped runs
    dst_off, p = [], MARGIN + 3
    for k, (s, e) in enumerate(runs):
        dst_off.append(p)
        p += int(seg_len[s:e].sum()) + (k % 3 == 0)  # back to back, a 1-byte canary after every third
    size = p + MARGIN
    got = pack(ctx, d, seg_off, seg_len, first, dst_off, size)
    same(got, image(host, seg_off, seg_len, runs, dst_off, size, size), "runs")


def test_no_segments_and_no_blocks(ctx, payload):
    host, d = payload
    dst = torch.full((1024,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.pack_device(d.data_ptr(), None, None, u64([0, 5, BIG, 1]), dst.data_ptr(), 1024, u64([300, 301, 2**50]), count=3,
                    nseg=0)  # nseg == 0: null segment arrays, every block empty
    ctx.pack_device(d.data_ptr(), u64([0]), u64([64]), u64([0]), dst.data_ptr(), 1024, u64([300]), count=0, nseg=1)
    ctx.pack_device(None, None, None, None, None, 0, None, count=0, nseg=0)
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all())
    with pytest.raises(kvsep.KvsepError):
        ctx.pack_device(d.data_ptr(), u64([0]), u64([64]), None, dst.data_ptr(), 1024, u64([300]), count=1, nseg=1)
    with pytest.raises(kvsep.KvsepError):
        ctx.pack_device(d.data_ptr(), None, u64([64]), u64([0, 1]), dst.data_ptr(), 1024, u64([300]), count=1, nseg=1)
    with pytest.raises(kvsep.KvsepError):
        ctx.pack_device(d.data_ptr(), u64([0]), u64([64]), u64([0, 1]), dst.data_ptr(), 1024, u64([300]), count=2**32,
                        nseg=1)


# ---------------------------------------------------------------- tiles
def test_lengths_around_the_tile(ctx, payload):
    host, d = payload
    lens = [T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T + 5, 7, T + 1]  # short blocks between and after the long ones
    seg_off = np.array([1, 70003, 200005, 300007, 500009, 700011, 13, 1000003], np.uint64)  # odd source alignments
    seg_len = np.array(lens, np.uint64)
    first = np.arange(len(lens) + 1, dtype=np.uint64)
    dst_off, p = [], MARGIN + 5
    for n in lens:
        dst_off.append(p)
        p += n  # back to back from an odd offset: every alignment pair differs
    size = p + MARGIN
    got = pack(ctx, d, seg_off, seg_len, first, dst_off, size)
    same(got, image(host, seg_off, seg_len, runs_of(first, len(lens)), dst_off, size, size), "tiles")


def test_one_long_block_alone(ctx):
    n = (8 << 20) + 13
    host = splitmix64_bytes(n + 4096, 99, 0)
    d = dev8(host)
    cuts = [0, 2_000_003, 2_000_003 + 4_194_309, n]  # three segments cut at odd places, laid out of order in the source
    seg_len = np.diff(cuts).astype(np.uint64)
    seg_off = np.array([int(seg_len[1]) + 7, 3, int(seg_len[0] + seg_len[1]) + 9], np.uint64)
    assert int(seg_off[2] + seg_len[2]) <= host.size
    first, dst_off, size = np.array([0, 3], np.uint64), [MARGIN + 11], MARGIN + 11 + n + MARGIN
    got = pack(ctx, d, seg_off, seg_len, first, dst_off, size)
    same(got, image(host, seg_off, seg_len, [(0, 3)], dst_off, size, size), "8 MiB + 13")


# ---------------------------------------------------------------- fit
@pytest.mark.parametrize("last_len", [100, 3 * 64 * 1024 + 1], ids=["short_last", "long_last"])
def test_a_record_that_does_not_fit_is_not_written(ctx, payload, last_len):
    host, d = payload
    seg_len = np.array([500, 0, 70000, 33, last_len], np.uint64)
    seg_off = np.array([9, 0, 1001, 200003, 300001], np.uint64)
    first = np.arange(6, dtype=np.uint64)
    dst_off = MARGIN + np.concatenate([[0], np.cumsum(seg_len[:-1])]).astype(np.uint64)
    end = int(dst_off[-1]) + last_len
    size = end + MARGIN
    runs = runs_of(first, 5)
    got = pack(ctx, d, seg_off, seg_len, first, dst_off, size, dst_bytes=end - 1)  # one byte short of the last record
    exp = image(host, seg_off, seg_len, runs, dst_off, size, end - 1)
    assert (exp[int(dst_off[-1]):] == CANARY).all()
    same(got, exp, "one byte short")
    got = pack(ctx, d, seg_off, seg_len, first, dst_off, size, dst_bytes=end)  # exact: everything is written
    same(got, image(host, seg_off, seg_len, runs, dst_off, size, end), "exact")
    off2 = dst_off.copy()
    off2[1], off2[3] = BIG - 3, end + 1  # an offset near 2^64 and one past dst_bytes: neither block is written
    got = pack(ctx, d, seg_off, seg_len, first, off2, size, dst_bytes=end)
    same(got, image(host, seg_off, seg_len, runs, off2, size, end), "offsets out of range")


# ---------------------------------------------------------------- the CRC routes of the frame forms
ROUTES = ["narrow", "wide", "planned"]


def route_context(route, nblocks, max_len, total):
    """(context, max_len hint) that sends the CRC pass down one route: the unplanned narrow kernel, the unplanned wide
    kernel, or the planned path (max_len unknown, 1 KiB pieces: blocks are split and combined)."""
    c = kvsep.Context(0)
    if route == "narrow":
        c.set_kernel("narrow")
        assert "narrow" in c.kernel_name(nblocks, max_len, total) and c.plan_query(nblocks, max_len, total)[1] == 0
        return c, max_len
    if route == "wide":
        c.set_kernel("wide")
        assert c.kernel_name(nblocks, max_len, total) == "crc32c_pieces_kernel"
        assert c.plan_query(nblocks, max_len, total)[1] == 0
        return c, max_len
    c.set_piece_bytes(1024)
    assert c.plan_query(nblocks, 0, total)[1] > 0  # blocks are split into pieces and combined
    return c, 0


def three_segments(payloads, rng):
    """Every payload as three segments at odd cuts, the segments scattered over a shuffled source buffer."""
    pieces = []
    for p in payloads:
        n = len(p)
        a = min(n, (n // 3) | 1)
        b = min(n, max(a, (2 * n // 3) | 1))
        pieces += [p[:a], p[a:b], p[b:]]
    seg_len = np.array([len(x) for x in pieces], np.uint64)
    seg_off, at = np.zeros(len(pieces), np.uint64), 0
    for j in rng.permutation(len(pieces)):
        at += int(rng.integers(0, 40))
        seg_off[j] = at
        at += len(pieces[j])
    src = splitmix64_bytes(at + 64, 5, 0)
    for j, x in enumerate(pieces):
        src[int(seg_off[j]):int(seg_off[j]) + len(x)] = np.frombuffer(x, np.uint8)
    return src, seg_off, seg_len, np.arange(0, len(pieces) + 1, 3, dtype=np.uint64)


@pytest.fixture(scope="module")
def small_vlog():
    with open(os.path.join(HERE, "ref_small.vlog"), "rb") as f:
        img = f.read()
    off, ln, stored, used = kvsep.vlog_walk(img)
    assert used == len(img) and off.size >= 10 and int(ln.max()) > T  # a payload of more than one tile among them
    payloads = [img[int(o):int(o + n)] for o, n in zip(off, ln)]
    src, seg_off, seg_len, first = three_segments(payloads, np.random.default_rng(21))
    return img, ln, payloads, src, seg_off, seg_len, first


def vlog_frame(c, d_src, seg_off, seg_len, first, rec_off, size, max_len, stream=None):
    nseg, count = len(seg_len), len(first) - 1
    seg_crc = torch.zeros(max(nseg, 1), dtype=torch.int32, device=DEV)
    crc_out = torch.zeros(max(count, 1), dtype=torch.int32, device=DEV)
    dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
    c.vlog_frame_device(d_src.data_ptr(), u64(seg_off), u64(seg_len), u64(first), seg_crc, crc_out, dst.data_ptr(), size,
                        u64(rec_off), count=count, nseg=nseg, total_bytes=int(seg_len.sum()), max_len=max_len)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), seg_crc.cpu().numpy().view(np.uint32)[:nseg], crc_out.cpu().numpy().view(np.uint32)[:count]


@pytest.fixture(scope="module")
def vlog_images():
    return {}


@pytest.mark.parametrize("route", ROUTES)
def test_vlog_frame_reproduces_the_reference_file(oracle, small_vlog, vlog_images, route):
    img, ln, payloads, src, seg_off, seg_len, first = small_vlog
    rec_off, end = kvsep.vlog_frame_offsets(ln, MARGIN)
    assert end == MARGIN + len(img)
    size = end + MARGIN
    c, hint = route_context(route, len(seg_len), int(seg_len.max()), int(seg_len.sum()))
    try:
        got, seg_crc, crc_out = vlog_frame(c, dev8(src), seg_off, seg_len, first, rec_off, size, hint)
        assert (got[:MARGIN] == CANARY).all() and (got[end:] == CANARY).all()
        same(got[MARGIN:end], np.frombuffer(img, np.uint8), route)  # the reference VlogWriter's file, byte for byte
        assert crc_out.tolist() == [oracle.extend(0, p) for p in payloads]
        assert np.array_equal(seg_crc, oracle.batch(src, seg_off, seg_len))
        n = len(payloads)
        assert c.vlog_verify(got[MARGIN:end].tobytes()) == (n, n, len(img))
        vlog_images[route] = got
        for other in vlog_images.values():  # the pack output does not depend on the route
            assert np.array_equal(other, got)
    finally:
        c.close()


def test_vlog_frame_equals_the_host_form(ctx):
    rng = np.random.default_rng(23)
    lens = rng.integers(0, 9001, 2000)
    lens[[0, 5, 1999]] = [0, 9000, 0]
    data = splitmix64_bytes(int(lens.sum()) + 1, 31, 0)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    payloads = [data[cuts[i]:cuts[i + 1]].tobytes() for i in range(lens.size)]
    want = np.frombuffer(ctx.vlog_frame(payloads), np.uint8)
    src, seg_off, seg_len, first = three_segments(payloads, rng)
    rec_off, end = kvsep.vlog_frame_offsets(lens.astype(np.uint64), MARGIN)
    got, _, _ = vlog_frame(ctx, dev8(src), seg_off, seg_len, first, rec_off, end + MARGIN, int(seg_len.max()))
    assert end - MARGIN == want.size
    assert (got[:MARGIN] == CANARY).all() and (got[end:] == CANARY).all()
    same(got[MARGIN:end], want, "host form")


@pytest.fixture(scope="module")
def sst_images():
    return {}


@pytest.mark.parametrize("route", ROUTES)
def test_sst_frame_reproduces_the_reference_file(sst_images, route):
    with open(os.path.join(HERE, "ref_table.sst"), "rb") as f:
        sst = np.frombuffer(f.read(), np.uint8)
    with open(os.path.join(HERE, "ref_framing.json")) as f:
        blocks = json.load(f)["sst"]["blocks"]
    off = np.array([b[0] for b in blocks], np.uint64)
    ln = np.array([b[1] for b in blocks], np.uint64)
    types = np.array([b[2] for b in blocks], np.uint8)
    rng = np.random.default_rng(29)
    src_off, at = np.zeros(len(blocks), np.uint64), 0
    for j in rng.permutation(len(blocks)):  # the blocks alone, scattered in shuffled order at every alignment
        at += int(rng.integers(1, 40))
        src_off[j] = at
        at += int(ln[j])
    src = splitmix64_bytes(at + 64, 7, 0)
    for j in range(len(blocks)):
        src[int(src_off[j]):int(src_off[j] + ln[j])] = sst[int(off[j]):int(off[j] + ln[j])]
    end = int((off + ln).max()) + 5
    size = MARGIN + end + MARGIN
    exp = np.full(size, CANARY, np.uint8)
    for o, n in zip(off, ln):  # the region of the file the handles cover: [block][type][trailer word]
        exp[MARGIN + int(o):MARGIN + int(o + n) + 5] = sst[int(o):int(o + n) + 5]
    c, hint = route_context(route, len(blocks), int(ln.max()), int(ln.sum()))
    try:
        dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
        masked = torch.zeros(len(blocks), dtype=torch.int32, device=DEV)
        d_src, d_len = dev8(src), u64(ln)
        c.sst_frame_device(d_src.data_ptr(), u64(src_off), d_len, dev8(types), masked, dst.data_ptr(), size,
                           u64(off + np.uint64(MARGIN)), total_bytes=int(ln.sum()), max_len=hint)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        same(got, exp, route)
        want = [int.from_bytes(bytes.fromhex(b[3]), "little") for b in blocks]
        assert masked.cpu().numpy().view(np.uint32).tolist() == want
        out = torch.zeros(len(blocks), dtype=torch.int32, device=DEV)
        fb = torch.zeros(1, dtype=torch.int64, device=DEV)
        nb = torch.ones(1, dtype=torch.int64, device=DEV)
        c.sst_verify_device(dst.data_ptr() + MARGIN, u64(off), d_len, out, fb, nb, max_len=int(ln.max()))
        torch.cuda.synchronize()
        assert (fb.item(), nb.item()) == (-1, 0)  # ReadBlock's check passes on every framed block
        sst_images[route] = got
        for other in sst_images.values():
            assert np.array_equal(other, got)
    finally:
        c.close()


# ---------------------------------------------------------------- capture
def test_captured_vlog_frame_replays_exactly(small_vlog):
    img, ln, payloads, src, seg_off, seg_len, first = small_vlog
    rec_off, end = kvsep.vlog_frame_offsets(ln, MARGIN)
    size, nseg, count, total = end + MARGIN, len(seg_len), len(ln), int(seg_len.sum())
    c = kvsep.Context(0)
    try:
        d_src, d_off, d_len, d_first, d_rec = dev8(src), u64(seg_off), u64(seg_len), u64(first), u64(rec_off)
        seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
        crc_out = torch.zeros(count, dtype=torch.int32, device=DEV)
        dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
        c.reserve(nseg, total)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.vlog_frame_device(d_src.data_ptr(), d_off, d_len, d_first, seg_crc, crc_out, dst.data_ptr(), size, d_rec,
                                total_bytes=total, max_len=0, stream=torch.cuda.current_stream())
        assert c.capture_sets()[1] == 1
        for poison in (0x00, 0xFF):
            dst.fill_(poison)
            crc_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert (got[:MARGIN] == poison).all() and (got[end:] == poison).all()
            same(got[MARGIN:end], np.frombuffer(img, np.uint8), f"replay over {poison:#x}")
        del g
        c.release_captures()
        assert c.capture_sets()[1] == 0
    finally:
        c.close()
