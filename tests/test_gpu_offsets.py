"""GPU: the offsets pass -- kvsep_crc32c_offsets_device (offsets_tile_sum_kernel, offsets_tile_scan_kernel,
offsets_write_kernel) -- exact against numpy cumsum:

  * counts 0, 1, 63, 64, 65, 1,023, 1,024, 1,025, 2,049 and 262,145 (one tile past 256 tiles: the scan kernel's
    per-thread runs hold two tiles), lengths 0..300, with no keep rule and keep all / none / alternating / random;
  * keep_before at 0, in the middle, at count and at ~0;
  * runs of 0, 1, 32, 33 and 1,500 segments (the serial and the wavefront sums), malformed first[] among them;
  * sums that reach 2^64, against a serial loop in Python integers;
  * canaries around dst_off, end and nkept in every case;
  * capture: a graph of verify_list -> salvage replayed with a different planted mismatch per replay, and the refusal of
    a captured call with more blocks than reserved.
"""
import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
SKIP = kvsep.OFFSET_SKIP
GUARD = 16
CANARY = 0x5A5A5A5A5A5A5A5A


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Out:
    """dst_off[count], end and nkept, each between canary words."""

    def __init__(self, count):
        self.count = count
        self.t = torch.full((count + 2 * GUARD + 2 + 2 * GUARD,), CANARY, dtype=torch.int64, device=DEV)
        base = self.t.data_ptr()
        self.dst_off = base + 8 * GUARD
        self.end = base + 8 * (2 * GUARD + count)
        self.nkept = base + 8 * (3 * GUARD + count + 1)

    def read(self):
        a = self.t.cpu().numpy().view(np.uint64)
        n, c = self.count, np.uint64(CANARY)
        guards = np.concatenate([a[:GUARD], a[GUARD + n:2 * GUARD + n], a[2 * GUARD + n + 1:3 * GUARD + n + 1],
                                 a[3 * GUARD + n + 2:]])
        assert guards.size == 4 * GUARD - 0 and (guards == c).all(), "a word around dst_off, end or nkept was written"
        return a[GUARD:GUARD + n], int(a[2 * GUARD + n]), int(a[3 * GUARD + n + 1])


def sizes_of(seg_len, first):
    """Block sizes under the documented clamp: both ends to nseg, a run that ends before it starts is empty."""
    if first is None:
        return seg_len.copy()
    nseg = seg_len.size
    pre = np.concatenate([[0], np.cumsum(seg_len, dtype=np.uint64)]).astype(np.uint64)
    s = np.minimum(first[:-1], nseg)
    e = np.maximum(np.minimum(first[1:], nseg), s)
    return pre[e.astype(np.int64)] - pre[s.astype(np.int64)]


def expected(size, kept, head, tail, start):
    ext = np.where(kept, size + np.uint64(head + tail), 0).astype(np.uint64)
    incl = np.cumsum(ext, dtype=np.uint64)
    off = np.where(kept, np.uint64(start) + incl - ext, np.uint64(SKIP)).astype(np.uint64)
    return off, start + int(incl[-1]) if size.size else start, int(np.count_nonzero(kept))


def check(ctx, seg_len, first, kept, head, tail, start, keep=None, keep_before=None, what=""):
    count = seg_len.size if first is None else first.size - 1
    o = Out(count)
    ctx.offsets_device(u64(seg_len), o.dst_off, o.end, first=None if first is None else u64(first),
                       keep=None if keep is None else dev8(keep),
                       keep_before=None if keep_before is None else u64([keep_before]), head=head, tail=tail,
                       start=start, nkept=o.nkept, count=count, nseg=seg_len.size)
    torch.cuda.synchronize()
    got_off, got_end, got_n = o.read()
    want_off, want_end, want_n = expected(sizes_of(seg_len, first), kept, head, tail, start)
    bad = np.flatnonzero(got_off != want_off)
    assert bad.size == 0, f"{what}: {bad.size} offsets differ, first at {bad[:5]}: {got_off[bad[:5]]} != {want_off[bad[:5]]}"
    assert (got_end, got_n) == (want_end, want_n), what


COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 262145]


@pytest.fixture(scope="module")
def lengths():
    return np.random.default_rng(20261020).integers(0, 301, max(COUNTS)).astype(np.uint64)


@pytest.mark.parametrize("count", COUNTS)
def test_counts_and_keep_masks(ctx, lengths, count):
    ln = lengths[:count]
    rng = np.random.default_rng(count)
    everything = np.ones(count, bool)
    check(ctx, ln, None, everything, 8, 0, 4096, what="no keep rule")
    masks = {"all": np.ones(count, np.uint8), "none": np.zeros(count, np.uint8),
             "alternating": (np.arange(count) % 2 * 0x80).astype(np.uint8),
             "random": (rng.integers(0, 3, count) * rng.integers(1, 120, count)).astype(np.uint8)}
    for name, keep in masks.items():
        check(ctx, ln, None, keep != 0, 0, 5, 0, keep=keep, what=f"keep {name}")


@pytest.mark.parametrize("count", [65, 2049])
def test_keep_before(ctx, lengths, count):
    ln = lengths[:count]
    for before in (0, 1, count // 2, count - 1, count, count + 7, SKIP):
        check(ctx, ln, None, np.arange(count) < min(before, count), 0, 0, 0, keep_before=before, what=f"before {before}")
    check(ctx, ln, None, np.zeros(count, bool), 0, 0, 77, keep_before=0, what="before 0, start 77")


def test_runs_short_and_long(ctx):
    """Runs of 0, 1, 32, 33 and 1,500 segments, several long ones in one 64-block row, over more than one tile; then
    the same segments under a first[] with decreasing and oversized values."""
    rng = np.random.default_rng(5)
    count = 1100
    run = rng.choice([0, 1, 32, 33, 1500, 2, 40], count, p=[.2, .3, .15, .15, .02, .1, .08])
    run[[0, 63, 64, 1023, 1024, 1099]] = [1500, 33, 33, 1500, 32, 33]
    first = np.concatenate([[0], np.cumsum(run)]).astype(np.uint64)
    seg_len = rng.integers(0, 5000, int(first[-1])).astype(np.uint64)
    keep = (rng.integers(0, 4, count) != 0).astype(np.uint8)
    check(ctx, seg_len, first, np.ones(count, bool), 8, 0, 12345, what="runs, no rule")
    check(ctx, seg_len, first, keep != 0, 0, 5, 0, keep=keep, what="runs, random keep")
    check(ctx, seg_len, first, np.arange(count) < 700, 8, 0, 0, keep_before=700, what="runs, keep_before")
    bent = first.copy()
    bent[[5, 70, 200, 1030]] = [first[9], SKIP, 0, seg_len.size + 3]  # decreasing, oversized: clamped, never followed
    check(ctx, seg_len, bent, keep != 0, 8, 5, 9, keep=keep, what="malformed first[]")
    check(ctx, seg_len[:0], np.zeros(count + 1, np.uint64), np.ones(count, bool), 8, 0, 0, what="no segments at all")


def test_sums_that_reach_2_64_mark_the_block_and_every_later_one(ctx):
    count = 1300
    ln = np.full(count, 10, np.uint64)
    ln[[3, 700, 1200]] = [2**63, 2**63 - 100, 2**62]
    for keep3, start in ((1, 0), (0, 0), (0, 2**62), (1, 2**64 - 2)):
        keep = np.ones(count, np.uint8)
        keep[3] = keep3
        keep[5::7] = 0
        pos, want, nk = start, [], 0
        for i in range(count):  # the contract, in Python integers
            if not keep[i]:
                want.append(SKIP)
                continue
            nk += 1
            e = min(pos + int(ln[i]) + 5, SKIP)
            want.append(SKIP if e == SKIP else pos)
            pos = e
        o = Out(count)
        ctx.offsets_device(u64(ln), o.dst_off, o.end, keep=dev8(keep), tail=5, start=start, nkept=o.nkept)
        torch.cuda.synchronize()
        got_off, got_end, got_n = o.read()
        assert got_off.tolist() == want and (got_end, got_n) == (pos, nk), (keep3, start)
        assert (pos == SKIP) == bool(keep3 or start), "the cases are meant to cross 2^64, all but one"


def test_nkept_is_optional_and_both_rules_are_refused(ctx):
    ln = np.arange(100, dtype=np.uint64)
    o = Out(100)
    ctx.offsets_device(u64(ln), o.dst_off, o.end)
    torch.cuda.synchronize()
    off, end, nk = o.read()
    assert end == int(ln.sum()) and nk == CANARY and off[99] == end - 99
    with pytest.raises(kvsep.KvsepError, match="both keep and keep_before"):
        ctx.offsets_device(u64(ln), o.dst_off, o.end, keep=dev8(np.ones(100)), keep_before=u64([5]))


# ---------------------------------------------------------------- capture
def planted(stored, bad):
    s = stored.copy()
    s[bad] ^= np.uint32(0x40)
    return s


def test_captured_verify_list_then_salvage_follows_each_replay(oracle):
    """check -> choose -> lay out -> copy in one graph: the stored words change between replays, and each replay's
    destination holds exactly the blocks that passed in that replay."""
    rng = np.random.default_rng(9)
    n = 2049
    ln = rng.integers(0, 600, n).astype(np.uint64)
    off = (np.concatenate([[0], np.cumsum(ln + np.uint64(3))[:-1]])).astype(np.uint64)
    total = int(ln.sum())
    src = splitmix64_bytes(int(off[-1] + ln[-1]) + 64, 99, 0)
    good = np.array([kvsep.mask(int(x)) for x in oracle.batch(src, off, ln, None, threads=4)], np.uint32)
    c = kvsep.Context(0)
    try:
        d_src, d_off, d_len = dev8(src), u64(off), u64(ln)
        stored = torch.zeros(n, dtype=torch.int32, device=DEV)
        out = torch.zeros(n, dtype=torch.int32, device=DEV)
        ok = torch.zeros(n, dtype=torch.uint8, device=DEV)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        dst = torch.zeros(total + 256, dtype=torch.uint8, device=DEV)
        o = Out(n)
        c.reserve(n, total)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            c.verify_list_device(d_src.data_ptr(), d_off, d_len, stored, out, res[0:1], res[1:2], ok=ok,
                                 total_bytes=total, max_len=600, stream=s)
            c.salvage_device(d_src.data_ptr(), d_off, d_len, dst.data_ptr(), total + 256, o.dst_off, o.end, keep=ok,
                             nkept=o.nkept, stream=s)
        assert c.capture_sets()[1] == 1
        for bad in ([], [0], [1024, 2048], list(range(0, n, 3)), list(range(n))):
            stored.copy_(torch.from_numpy(planted(good, bad).view(np.int32)))
            dst.fill_(0xA5)
            g.replay()
            torch.cuda.synchronize()
            kept = np.ones(n, bool)
            kept[bad] = False
            want_off, want_end, want_n = expected(ln, kept, 0, 0, 0)
            got_off, got_end, got_n = o.read()
            assert np.array_equal(got_off, want_off) and (got_end, got_n) == (want_end, want_n), len(bad)
            parts = [src[int(a):int(a + b)] for a, b, k in zip(off, ln, kept) if k]
            want = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
            got = dst.cpu().numpy()
            assert np.array_equal(got[:want_end], want) and (got[want_end:] == 0xA5).all(), len(bad)
            assert int(res[1].item()) == len(bad)
        big, d_big = Out(n + 1), u64(np.ones(n + 1))
        torch.cuda.synchronize()
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):  # more blocks than reserved: refused at capture
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                c.offsets_device(d_big, big.dst_off, big.end, stream=torch.cuda.current_stream())
        del g2
        torch.cuda.synchronize()
        assert (big.t.cpu().numpy().view(np.uint64) == np.uint64(CANARY)).all()  # nothing was enqueued
        del g
        c.release_captures()
    finally:
        c.close()
