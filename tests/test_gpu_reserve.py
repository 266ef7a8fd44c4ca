"""GPU: kvsep_crc32c_reserve's promise, the automatic piece sizes and the SST device forms where no other test goes.

include/kvsep_crc32c.h: after reserve(count, total_bytes) no call of up to that many blocks and bytes allocates, so it
can be captured into a graph -- the planned, narrow, verify and SST forms alike.  The plan of a batch depends on its
piece size, and a fresh context picks 128, 64, 32 or 16 KiB pieces by the batch's total (csrc/plan_size.h): a batch one
byte under a threshold want * P takes P / 2 pieces and needs twice the plan entries, and the SST read check runs
len + 1 bytes per block.  Here:

  * eager batches and verify calls exactly on and one byte under every threshold, with block lengths around the
    multiples of both piece sizes, on all three schedules;
  * captured batches of every smaller size after one reserve(n, T);
  * the SST trailer and read-check forms captured into one graph with the caller's own reserve(count, sum(len)), on
    the planned, claim, sorted-window and wide routes, clean, damaged and repaired;
  * the eager SST read check at the shape it exists for -- 4 KiB blocks with a 4 KiB hint, which it runs as 4,097-byte
    blocks -- on both sides of the claim kernel's two count bounds.

Every test makes a fresh context and never sets a piece size, and asserts through kvsep_crc32c_plan_query
(csrc/kvsep_testing.h) and kernel_name that it ran the piece size, schedule and kernel it meant to.  Expected values
come from the oracle on the same bytes."""
import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
NONE = 2**64 - 1
KiB, MiB = 1 << 10, 1 << 20
POOL = 8 * MiB
WANT = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8  # plan_size.h want_pieces
SMALL = [0, 1, 15, 16, 17]


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def mask(crc):
    """leveldb::crc32c::Mask (util/crc32c.h:29) on a uint32 array."""
    c = np.asarray(crc, np.uint32)
    return ((c >> np.uint32(15)) | (c << np.uint32(17))) + np.uint32(kvsep.MASK_DELTA)


def verdict(fb, nb):
    return int(fb.item()) & NONE, int(nb.item())


@pytest.fixture(scope="module")
def pool():
    """One 8 MiB splitmix64 pool, host and device: every batch lays its (overlapping) blocks over it."""
    host = splitmix64_bytes(POOL, 0x7E5E77E, 0)
    return host, torch.from_numpy(host).to(DEV)


def edge_lengths(piece):
    """Lengths around the multiples of `piece` and of its half: where a block gains a piece under either size."""
    out = []
    for q in (piece, piece // 2):
        for k in (1, 2, 3, 5):
            out += [k * q - 1, k * q, k * q + 1, k * q + 33]
        out += [2 * q - 16, 2 * q + 15]
    return out + SMALL


def layout(target, edges, seed):
    """Blocks at odd pool offsets whose lengths sum to exactly `target`: the edge lengths that fit, then fillers of
    about 1 MiB, the last one cut to make the sum; shuffled."""
    rng = np.random.default_rng(seed)
    ln, left = [], target
    for e in edges:
        if e <= left:
            ln.append(e)
            left -= e
    while left:
        f = min(left, MiB + int(rng.integers(-4096, 4097)))
        ln.append(f)
        left -= f
    ln = np.array(ln, np.uint64)
    rng.shuffle(ln)
    assert int(ln.sum()) == target and int(ln.max()) < POOL // 2
    off = rng.integers(0, (POOL - ln.astype(np.int64)) // 2).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    assert int((off + ln).max()) <= POOL
    return off, ln


class Batch:
    """A batch over the pool with its oracle CRCs (random 32-bit inits) and device arrays."""

    def __init__(self, pool, oracle, off, ln, seed):
        host, self.data = pool
        self.off, self.ln, self.n, self.total = off, ln, off.size, int(ln.sum())
        self.init = np.random.default_rng(seed).integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32)
        self.exp = oracle.batch(host, off, ln, self.init, threads=16)
        self.d_off, self.d_len, self.d_init = i64(off), i64(ln), i32(self.init)

    def planted(self, piece):
        """(stored words with `stored ^= 1` at four blocks, those blocks): block 0, the last, one single-piece block
        and the block with the most pieces."""
        pieces = np.maximum(self.ln // np.uint64(piece), np.uint64(1))
        single = next(i for i in range(1, self.n - 1) if pieces[i] == 1 and self.ln[i] > 0)
        most = int(np.argmax(pieces[1:self.n - 1])) + 1
        bad = sorted({0, self.n - 1, single, most})
        assert len(bad) == 4 and pieces[most] > 1
        stored = mask(self.exp)
        stored[bad] ^= np.uint32(1)
        return stored, bad

    def run_batch(self, ctx, out, **kw):
        ctx.batch_device(self.data.data_ptr(), self.d_off, self.d_len, out, init=self.d_init, total_bytes=self.total,
                         max_len=0, **kw)

    def run_verify(self, ctx, d_stored, out, fb, nb, **kw):
        ctx.verify_device(self.data.data_ptr(), self.d_off, self.d_len, d_stored, out, fb, nb, init=self.d_init,
                          total_bytes=self.total, max_len=0, **kw)


def check_eager(ctx, b, piece, guided_auto=None):
    """Batch form, then verify form with four planted mismatches, then a clean verify, on every schedule."""
    assert mask(np.array([0x12345678], np.uint32))[0] == kvsep.mask(0x12345678)
    out = torch.zeros(b.n, dtype=torch.int32, device=DEV)
    fb = torch.zeros(1, dtype=torch.int64, device=DEV)
    nb = torch.zeros(1, dtype=torch.int64, device=DEV)
    stored, bad = b.planted(piece)
    d_bad, d_clean = i32(stored), i32(mask(b.exp))
    for sched in (None, False, True):
        ctx.set_schedule(sched)
        got_piece, needed, guided = ctx.plan_query(b.n, 0, b.total)
        assert (got_piece, needed) == (piece, b.n + b.total // piece + 1), (sched, got_piece, needed)
        if sched is not None or guided_auto is not None:
            assert guided == (guided_auto if sched is None else sched), (sched, guided)
        out.zero_()
        b.run_batch(ctx, out)
        torch.cuda.synchronize()
        assert np.array_equal(u32(out), b.exp), (sched, np.flatnonzero(u32(out) != b.exp)[:8])
        out.zero_()
        b.run_verify(ctx, d_bad, out, fb, nb)
        torch.cuda.synchronize()
        assert verdict(fb, nb) == (0, 4), (sched, verdict(fb, nb), bad)
        assert np.array_equal(u32(out), b.exp), sched
        b.run_verify(ctx, d_clean, out, fb, nb)
        torch.cuda.synchronize()
        assert verdict(fb, nb) == (NONE, 0), (sched, verdict(fb, nb))


@pytest.mark.parametrize("under", [0, 1], ids=["at", "under"])
@pytest.mark.parametrize("piece_kib", [32, 64, 128])
def test_auto_piece_thresholds_eager(piece_kib, under, pool, oracle):
    """sum(len) = want * P picks P-byte pieces, want * P - 1 picks P / 2."""
    P = piece_kib * KiB
    off, ln = layout(WANT * P - under, edge_lengths(P), 1000 + piece_kib + under)
    b = Batch(pool, oracle, off, ln, 7 + piece_kib)
    ctx = kvsep.Context(0)
    try:
        check_eager(ctx, b, P // 2 if under else P)
    finally:
        ctx.close()


def test_guided_schedule_on_small_pieces(pool, oracle):
    """About 12,000 blocks (on 256 CUs) of 1..40,000 bytes, between the 32 and 64 KiB thresholds: 32 KiB pieces, and
    enough items that the automatic schedule is the guided one -- the guided schedule on a small-piece table."""
    rng = np.random.default_rng(4242)
    n = WANT * 293 // 100
    ln = rng.integers(1, 40001, n).astype(np.uint64)
    assert WANT * 32 * KiB <= int(ln.sum()) < WANT * 64 * KiB
    off = rng.integers(0, (POOL - 70000) // 2, n).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    ln[:len(SMALL)] = SMALL
    ln[len(SMALL):len(SMALL) + 4] = [32 * KiB - 1, 32 * KiB, 32 * KiB + 1, 64 * KiB + 33]  # more than one piece
    b = Batch(pool, oracle, off, ln, 99)
    ctx = kvsep.Context(0)
    try:
        assert ctx.plan_query(b.n, 0, b.total) == (32 * KiB, b.n + b.total // (32 * KiB) + 1, True)
        check_eager(ctx, b, 32 * KiB, guided_auto=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("piece_kib", [32, 64, 128])
def test_captured_batches_below_the_reserved_size(piece_kib, pool, oracle):
    """After reserve(n, T) with T = want * P, a batch of any smaller total captures -- T - 1 and below pick smaller
    pieces and need more plan entries than a plan of P-byte pieces for T holds -- and replays exactly, twice."""
    P = piece_kib * KiB
    T = WANT * P
    edges = [P - 1, P, P + 1, 2 * P + 15, P // 2 + 1, 3 * (P // 2) - 1, 5 * (P // 4) + 33] + SMALL
    batches = [Batch(pool, oracle, *layout(t, edges, 50 + k), seed=60 + k)
               for k, t in enumerate([T, T - 1, T // 2, T // 2 - 1, T // 4 - 1, MiB])]
    n = max(b.n for b in batches)
    vb = batches[1]  # the verify-form graph: one byte under the threshold
    ctx = kvsep.Context(0)
    try:
        ctx.reserve(n, T)
        ctx.reserve_captures(len(batches) + 1)
        assert ctx.plan_query(batches[0].n, 0, T)[0] == P and ctx.plan_query(vb.n, 0, T - 1)[0] == P // 2
        vpiece = ctx.plan_query(vb.n, 0, vb.total)[0]
        stored, bad = vb.planted(vpiece)
        d_stored = i32(stored)
        fb = torch.zeros(1, dtype=torch.int64, device=DEV)
        nb = torch.zeros(1, dtype=torch.int64, device=DEV)
        outs = [torch.zeros(b.n, dtype=torch.int32, device=DEV) for b in batches]
        vout = torch.zeros(vb.n, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        graphs = []
        for b, out in zip(batches, outs):  # one call per graph, each on a capture set of its own
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                b.run_batch(ctx, out, stream=torch.cuda.current_stream())
            graphs.append(g)
        vg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(vg):
            vb.run_verify(ctx, d_stored, vout, fb, nb, stream=torch.cuda.current_stream())
        assert ctx.capture_sets() == (len(batches) + 1, len(batches) + 1)
        for rnd in range(2):
            for b, out, g in zip(batches, outs, graphs):
                out.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(u32(out), b.exp), (rnd, b.total, np.flatnonzero(u32(out) != b.exp)[:8])
            vout.zero_()
            fb.fill_(7)
            nb.fill_(7)
            vg.replay()
            torch.cuda.synchronize()
            assert verdict(fb, nb) == (0, 4), (rnd, verdict(fb, nb), bad)
            assert np.array_equal(u32(vout), vb.exp), rnd
        del graphs, vg, g
        torch.cuda.synchronize()
        ctx.release_captures()
        assert ctx.capture_sets()[1] == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the SST forms
def sst_file(lens, seed, oracle):
    """An SST file image as framing_builders.sst_image lays it out -- block, type byte, Mask(crc of block + type) LE32,
    back to back -- built array-wise, checksums from the oracle; the payload bytes are generated on the device (a
    quarter of a gigabyte takes seconds on the host).  -> (device image, off, types, stored words, unmasked CRCs)"""
    lens = np.asarray(lens, np.uint64)
    off = np.zeros(lens.size, np.uint64)
    off[1:] = np.cumsum(lens[:-1] + np.uint64(5), dtype=np.uint64)
    nbytes = int(off[-1] + lens[-1]) + 5 + 64
    d = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    kvsep.fill_splitmix64(d.data_ptr(), nbytes, seed, 0)
    torch.cuda.synchronize()
    img = d.cpu().numpy()
    types = np.random.default_rng(seed).integers(0, 2, lens.size).astype(np.uint8)  # kNoCompression / kSnappy
    t_at = (off + lens).astype(np.int64)
    img[t_at] = types
    crc = oracle.batch(img, off, lens + np.uint64(1), threads=16)
    words = mask(crc)
    for j in range(4):
        img[t_at + 1 + j] = ((words >> np.uint32(8 * j)) & np.uint32(0xFF)).astype(np.uint8)
    d.copy_(torch.from_numpy(img))
    return d, off, types, words, crc


def sst_shape(kind):
    rng = np.random.default_rng(31)
    if kind == "planned":  # ragged blocks, no hint; sum(len) = 16,383 mod 16 KiB: the type bytes cross a piece boundary
        ln = rng.integers(1, 8193, 3000).astype(np.uint64)
        ln[-1] += np.uint64((16383 - int(ln.sum())) % (16 * KiB))
        assert int(ln.sum()) % (16 * KiB) == 16383
        return ln, 0
    if kind == "claim":
        return np.full(32768, 4096, np.uint64), 4096
    if kind == "sorted":
        return rng.integers(1, 4097, 30000).astype(np.uint64), 4096
    return np.full(2000, 70_000, np.uint64), 70_000  # wide: one wave per unsplit block


@pytest.mark.parametrize("kind", ["planned", "claim", "sorted", "wide"])
def test_captured_sst_forms(kind, oracle):
    """sst_trailers_device, then sst_verify_device, captured into one graph after reserve(count, sum(len)) with the
    caller's own numbers; replayed on the clean file, with three blocks damaged in device memory, and repaired."""
    ln, hint = sst_shape(kind)
    d, off, types, words, crc = sst_file(ln, 77, oracle)
    n, total = ln.size, int(ln.sum())
    d_off, d_len, d_types = i64(off), i64(ln), torch.from_numpy(types).to(DEV)
    masked = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    fb = torch.zeros(1, dtype=torch.int64, device=DEV)
    nb = torch.zeros(1, dtype=torch.int64, device=DEV)
    ctx = kvsep.Context(0)
    try:
        # the route of the read check's own call: len + 1 per block under hint + 1
        name = ctx.kernel_name(n, hint + 1 if hint else 0, total + n)
        needed = ctx.plan_query(n, hint + 1 if hint else 0, total + n)[1]
        if kind == "planned":
            piece = ctx.plan_query(n, 0, total + n)[0]
            assert needed == n + (total + n) // piece + 1 and name == "crc32c_pieces_kernel"
            if piece == 16 * KiB:  # (on any device of up to 2,900 CUs)
                assert needed > n + total // piece + 1  # more than a plan for the caller's total_bytes holds
        elif kind == "wide":
            assert needed == 0 and name == "crc32c_pieces_kernel"
        else:
            assert needed == 0 and kind in name, name
            assert kind in ctx.kernel_name(n, hint, total)  # the trailer form's call
        ctx.reserve(n, total)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            ctx.sst_trailers_device(d.data_ptr(), d_off, d_len, d_types, masked, total_bytes=total, max_len=hint,
                                    stream=s)
            ctx.sst_verify_device(d.data_ptr(), d_off, d_len, out, fb, nb, total_bytes=total, max_len=hint, stream=s)
        assert ctx.capture_sets()[1] == 1  # both calls on the graph's one set

        def replay():
            masked.zero_()
            out.zero_()
            fb.fill_(7)
            nb.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            return u32(masked), u32(out), (int(fb.item()), int(nb.item()))

        def clean(tag):
            m, o, v = replay()
            assert v == (-1, 0), (tag, v)
            assert np.array_equal(m, words), (tag, np.flatnonzero(m != words)[:8])
            assert np.array_equal(o, crc), (tag, np.flatnonzero(o != crc)[:8])

        clean("clean")
        mid = n // 2
        at = [int(off[0]) + int(ln[0]) // 2, int(off[mid] + ln[mid]), int(off[-1] + ln[-1]) + 3]
        saved = [int(d[a].item()) for a in at]
        d[at[0]] ^= 0x40        # a payload byte of block 0
        d[at[1]] ^= 0x01        # the type byte of a middle block: in the file, and as the writer passes it
        d_types[mid] ^= 0x01
        d[at[2]] ^= 0x80        # the stored word of the last block
        m, o, v = replay()
        assert v == (0, 3), v
        assert m[0] != words[0] and m[mid] != words[mid]
        same = np.ones(n, bool)
        same[[0, mid]] = False
        assert np.array_equal(m[same], words[same]) and np.array_equal(o[same], crc[same])
        assert o[0] != crc[0] and o[mid] != crc[mid]
        for a, v0 in zip(at, saved):
            d[a] = v0
        d_types[mid] ^= 0x01
        clean("repaired")
        del g
        torch.cuda.synchronize()
        ctx.release_captures()
    finally:
        ctx.close()


CFG2_LEN = 4096
CFG2_COUNTS = [32767, 32768, 65536, 65537]


@pytest.fixture(scope="module")
def cfg2_file(oracle):
    """65,537 blocks of 4 KiB with their 5-byte trailers: every count below is a prefix of it."""
    n = max(CFG2_COUNTS)
    d, off, types, words, crc = sst_file(np.full(n, CFG2_LEN, np.uint64), 2024, oracle)
    return dict(d=d, off=off, types=types, words=words, crc=crc)


def cfg2_read_check_kernel(count):
    """route::decide (csrc/route.h) for the read check's call of uniform 4,097-byte blocks under a 4,097
    hint: the claim kernel from 1 << 15 blocks up to 1 << 16 (the bound for max_len > 4 KiB), else the narrow kernel
    (16-wave below 1 << 17 blocks)."""
    return "crc32c_narrow_claim_kernel" if (1 << 15) <= count <= (1 << 16) else "crc32c_narrow_kernel"


@pytest.mark.parametrize("count", CFG2_COUNTS)
def test_sst_verify_at_config2_routing_edges(count, cfg2_file):
    """Config 2's read check (table/format.cc:99-106 over 4 KiB blocks, 4 KiB hint) on each side of the claim
    kernel's lower and upper count bounds: every CRC and trailer word, exact verdicts for mismatches at the batch's
    ends, at both ends of an 8-block group and around the last group, and for every block bad."""
    f = cfg2_file
    total = count * CFG2_LEN
    stride = CFG2_LEN + 5
    d = f["d"]
    d_off, d_len = i64(f["off"][:count]), i64(np.full(count, CFG2_LEN, np.uint64))
    d_types = torch.from_numpy(f["types"][:count]).to(DEV)
    words, crc = f["words"][:count], f["crc"][:count]
    masked = torch.zeros(count, dtype=torch.int32, device=DEV)
    out = torch.zeros(count, dtype=torch.int32, device=DEV)
    fb = torch.zeros(1, dtype=torch.int64, device=DEV)
    nb = torch.zeros(1, dtype=torch.int64, device=DEV)
    ctx = kvsep.Context(0)
    try:
        assert ctx.kernel_name(count, CFG2_LEN + 1, total + count) == cfg2_read_check_kernel(count)
        assert ctx.plan_query(count, CFG2_LEN + 1, total + count)[1] == 0

        def check():
            out.zero_()
            fb.fill_(7)
            nb.fill_(7)
            ctx.sst_verify_device(d.data_ptr(), d_off, d_len, out, fb, nb, total_bytes=total, max_len=CFG2_LEN)
            torch.cuda.synchronize()
            assert np.array_equal(u32(out), crc), np.flatnonzero(u32(out) != crc)[:8]
            return int(fb.item()), int(nb.item())

        ctx.sst_trailers_device(d.data_ptr(), d_off, d_len, d_types, masked, total_bytes=total, max_len=CFG2_LEN)
        torch.cuda.synchronize()
        assert np.array_equal(u32(masked), words), np.flatnonzero(u32(masked) != words)[:8]
        assert check() == (-1, 0)
        k = count // 16
        bad = sorted({0, count - 1, 8 * k, 8 * k + 7, count - 8, count - 9})
        at = torch.tensor([b * stride + CFG2_LEN + 2 for b in bad], device=DEV)  # a byte of each stored word
        for lowest in (0, 1):  # with block 0 bad, then with it good: first_bad moves into the group
            sel = at[lowest:]
            d[sel] ^= 0x10
            got = check()
            d[sel] ^= 0x10
            assert got == (bad[lowest], len(bad) - lowest), (got, bad)
        stored = d[:count * stride].view(count, stride)[:, CFG2_LEN + 1]
        stored ^= 0x01  # every stored word wrong
        got = check()
        stored ^= 0x01
        assert got == (0, count), got
        assert check() == (-1, 0)
    finally:
        ctx.close()
