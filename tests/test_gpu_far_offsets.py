"""GPU: the framing, layout and log forms with offsets and totals at and across 2^32.

Every other GPU test of these forms moves a few MiB from offset 0; the workload they were written for is a 512 GiB vlog
in 64 GiB slices, where seg_off, dst_off, rec_off, *end and dest_length are routinely above 2^32.  A kernel that kept a
position, a running sum or an address delta in 32 bits would pass all of them.  Two tiers:

  A  far offsets, few bytes moved: one source and one destination allocation of 5 GiB + 1 MiB; each case moves a few KiB
     to and from offsets just below, at and just above 2^32 and at the end of the allocation.
  B  totals that reach 2^32: a unit of 64 MiB + 3 bytes at an odd source offset, used as a segment many times, and a log
     image of 2^32 + 3 * 32,768 bytes made of a period of 129 blocks.

No expectation comes from a library form.  Byte images are built with numpy from a host copy of the source bytes (the
source is the splitmix stream of its own offset, so any window of it can be made on the host); CRCs come from the oracle
(a repeated unit by chaining oracle.extend_addr); layouts, log walks, verdicts, chains and record assembly from the pure
models of kv-separate_amd/tools/soak_forms.py and tests/framing_builders.py, run on a small window whose offsets are
then shifted to where the window lies (Windows below), or on one period shifted by the period's stride.  Large
destinations are compared on the device against an expected image made of a canary fill and the windows the model wrote,
which also proves that nothing else was written.  Everything is bit-exact.

What the ABI does not let a caller place far: kvsep_crc32c_salvage_device, kvsep_sst_salvage_device and
kvsep_log_records_device lay out from destination offset 0, and kvsep_log_frame_device writes from dst + 0 whatever
dest_length is.  Their far side is the source here (and, in tier B, the running total); the layout from a far `start` is
the offsets pass and the gather-copy as two calls.
"""
import os
import struct
import sys

import numpy as np
import pytest

import framing_builders as FB
import kvsep
from kvsep import splitmix64_bytes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kv-separate_amd", "tools"))
import soak_forms as S  # noqa: E402  (the pure models only: no runner, no generator)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
GiB, T32, U64 = 1 << 30, 1 << 32, (1 << 64) - 1
SKIP = kvsep.OFFSET_SKIP
CANARY = 0xA5
FAR_BYTES = 5 * GiB + (1 << 20)
SEED = 0x0FA20FF5
# block p of a group reads from S_OFF[(p + k) % 8] (segment k) and writes to D_OFF[p]: the same set rotated by three, so
# that source and destination alignment differ (mod 16: 15, 15, 15, 0, 1, 15, 3, 8)
S_OFF = [T32 - 4097, T32 - 17, T32 - 1, T32, T32 + 1, T32 + 15, T32 + 4099, 5 * GiB - 3000]
D_OFF = S_OFF[3:] + S_OFF[:3]
END = 5 * GiB - 3000


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev8(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).to(DEV)  # (a copy: a bytes object's view is read-only)


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def is_canary(t):
    return bool((t == CANARY).all())


class Windows:
    """Spans (far offset, bytes) of a large allocation laid back to back as one small array: near(x) is where far
    offset x lies in it.  The models run on the small array; their results are shifted back span by span."""

    def __init__(self, spans):
        self.spans, self.base, self.size = spans, [], 0
        for _, n in spans:
            self.base.append(self.size)
            self.size += n

    def near(self, x, n=0):
        if x == SKIP:
            return SKIP
        for (a, m), b in zip(self.spans, self.base):
            if a <= x and x + n <= a + m:
                return b + (x - a)
        raise AssertionError(f"[{x}, +{n}) lies in no window")

    def near_all(self, xs):
        return np.array([self.near(int(x)) for x in xs], np.uint64).reshape(len(xs))


SRC_WIN = Windows([(T32 - 65536, 131072), (5 * GiB - 65536, 65536 + (1 << 20))])
DST_WIN = Windows([(T32 - 16384, 49152), (5 * GiB - 16384, 16384 + (1 << 20))])


def case(form, inp, par, out=()):
    c = S.Case("far", 0, 0)
    c.form, c.inp, c.par, c.out = form, inp, dict(par, src_skew=0), {k: None for k in out}
    return c


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Far:
    """The tier A allocations: src (uninitialised but for the windows, whose byte at offset x is byte x of the splitmix
    stream), dst and the expected image `want` (canary)."""

    def __init__(self):
        self.src = torch.empty(FAR_BYTES, dtype=torch.uint8, device=DEV)
        for a, n in SRC_WIN.spans:
            kvsep.fill_splitmix64(self.src.data_ptr() + a, n, SEED, a)
        self.src_near = np.concatenate([splitmix64_bytes(n, SEED, a) for a, n in SRC_WIN.spans])
        self.dst = torch.empty(FAR_BYTES, dtype=torch.uint8, device=DEV)
        self.want = torch.empty(FAR_BYTES, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def reset(self):
        self.dst.fill_(CANARY)
        self.want.fill_(CANARY)

    def check(self, near_image, what):
        """dst against canary + the model's windows, on the device."""
        assert near_image.size == DST_WIN.size
        for (a, n), b in zip(DST_WIN.spans, DST_WIN.base):
            self.want[a:a + n] = dev8(near_image[b:b + n])
        if torch.equal(self.dst, self.want):
            return
        for lo in range(0, FAR_BYTES, GiB):  # the first difference, for the report
            d = (self.dst[lo:lo + GiB] != self.want[lo:lo + GiB]).nonzero()
            if d.numel():
                at = lo + int(d[0])
                raise AssertionError(f"{what}: dst[{at}] (2^32 {at - T32:+d}) = {int(self.dst[at])} "
                                     f"want {int(self.want[at])}; {int(d.numel())} bytes differ in this GiB")


@pytest.fixture(scope="module")
def far():
    f = Far()
    yield f
    del f.src, f.dst, f.want


# ------------------------------------------------------------------------------------------------- tier A: placement
def split_total(rng, total, k, top=3000):
    """k segment lengths of 0..top bytes that add up to total, some of them empty."""
    parts, left = [0] * k, total
    order = [int(j) for j in rng.permutation(k)]
    for idx, j in enumerate(order[:-1]):
        lo = max(0, left - top * (k - idx - 1))
        parts[j] = lo if rng.random() < 0.25 else int(rng.integers(lo, min(top, left) + 1))
        left -= parts[j]
    parts[order[-1]] = left
    assert 0 <= left <= top and sum(parts) == total
    return parts


# the destination offsets whose blocks carry bytes, per group: group 0 fills the gaps between all eight, the others
# leave room for one block that runs across 2^32
LIVE = [set(D_OFF), {T32 - 4097, T32 + 4099, END}, {T32 - 17, T32 + 4099, END}, {T32 - 1, T32 + 15, T32 + 4099, END},
        {T32 - 4097, T32, END}]


def placement(group, frame, one_segment=False, live=None):
    """One group's batch -> (seg_off, seg_len, first, dst_off, payload sizes), all far.  Block p goes to D_OFF[p]; a live
    block takes up to the bytes between it and the next live one (frame bytes included), from its own length upward when
    that makes it run across 2^32; the others are empty (plain: they write nothing) or not laid out (framed: a frame
    would not fit between two neighbours a byte apart).  Group 4 adds a block that ends exactly at dst_bytes, which must
    be written, and one that ends a byte later, which must not."""
    rng = np.random.default_rng([77, group, frame])
    live = sorted(LIVE[group] if live is None else live)
    while True:  # a framed block needs room for its frame
        tight = [d for d, nxt in zip(live, live[1:]) if nxt - d < frame]
        if not tight:
            break
        live.remove(tight[0])
    dsts = list(D_OFF) + [d for d in live if d not in D_OFF]
    seg_off, seg_len, first, dst_off, size = [], [], [0], [], []
    top = 3000

    def block(p, total, at):
        k = 1 if one_segment else int(rng.integers(max(1, -(-total // top)), 6))
        for j, ln in enumerate(split_total(rng, total, k)):
            seg_off.append(S_OFF[(p + j) % 8])
            seg_len.append(ln)
        first.append(len(seg_len))
        dst_off.append(at)
        size.append(total)

    for p, d in enumerate(dsts):
        if d not in live:
            if frame:
                block(p, int(rng.integers(0, 200)), SKIP)
            elif rng.random() < 0.3 and not one_segment:
                first.append(len(seg_len))  # no segments at all
                dst_off.append(d)
                size.append(0)
            else:
                block(p, 0, d)
            continue
        nxt = [x for x in live if x > d]
        cap = min((top if one_segment else 5 * top), (nxt[0] - d if nxt else 1 << 20) - frame)
        need = T32 - d + 1 if d < T32 and group else 0  # so many bytes, frame included, reach across 2^32
        lo = max(0, need - frame) if need - frame <= cap else 0
        block(p, int(rng.integers(lo, cap + 1)), d)
    if group == 4:
        for extra in (0, 1):
            total = int(rng.integers(1500, 2500))
            block(len(dst_off), total, FAR_BYTES - (total + frame) + extra)
    return (np.array(seg_off, np.uint64), np.array(seg_len, np.uint64), np.array(first, np.uint64),
            np.array(dst_off, np.uint64), np.array(size, np.uint64))


def near_inputs(far, seg_off, seg_len, dst_off):
    so = np.array([SRC_WIN.near(int(o), int(n)) if n else 0 for o, n in zip(seg_off, seg_len)], np.uint64)
    return dict(src=far.src_near, seg_off=so.reshape(seg_off.size), seg_len=seg_len, dst_off=DST_WIN.near_all(dst_off))


def reach(seg_off, seg_len, first, dst_off, size, frame):
    """Which of the cases the placement is there for a batch holds: a block with segments on both sides of 2^32 in the
    source, a block whose destination range runs across 2^32, a block that ends at dst_bytes and one a byte past it."""
    got = set()
    for i, d in enumerate(dst_off):
        d, n = int(d), int(size[i]) + frame
        segs = [(int(seg_off[j]), int(seg_len[j])) for j in range(int(first[i]), int(first[i + 1])) if seg_len[j]]
        if any(o + k <= T32 for o, k in segs) and any(o >= T32 for o, k in segs):
            got.add("both_sides")
        if any(o < T32 < o + k for o, k in segs):
            got.add("segment_across")
        if d == SKIP:
            continue
        if d < T32 < d + n:
            got.add("dst_across")
        if d + n == FAR_BYTES:
            got.add("ends_at_dst_bytes")
        if d + n == FAR_BYTES + 1:
            got.add("one_past_dst_bytes")
        if d + n <= FAR_BYTES:
            DST_WIN.near(d, n)  # a written range lies inside one window
    return got


@pytest.mark.parametrize("frame,one_segment", [(0, False), (8, False), (5, True)], ids=["plain", "vlog", "sst"])
def test_placement_reaches_the_cases(frame, one_segment):
    """The batches of the three tests below hold the cases they are there for (no device work)."""
    got = [reach(*placement(g, frame, one_segment), frame) for g in range(5)]
    for g in (2, 3) if one_segment else (1, 2, 3):
        assert "dst_across" in got[g], g
    assert {"ends_at_dst_bytes", "one_past_dst_bytes"} <= got[4]
    assert any("segment_across" in s for s in got)
    assert one_segment or any("both_sides" in s for s in got)


@pytest.mark.parametrize("group", range(5))
def test_pack_far_source_and_destination(ctx, far, group):
    """kvsep_crc32c_pack_device: blocks of 1..5 segments of 0..3,000 bytes (some empty, some blocks without a segment),
    read from and written to {2^32 - 4097, - 17, - 1, 2^32, + 1, + 15, + 4099, 5 * 2^30 - 3000}; blocks whose segments
    lie on both sides of 2^32, blocks written across 2^32, a block that ends at dst_bytes (written) and one that ends a
    byte past it (not written)."""
    seg_off, seg_len, first, dst_off, size = placement(group, 0)
    reach(seg_off, seg_len, first, dst_off, size, 0)
    n = dst_off.size
    c = case("pack", dict(near_inputs(far, seg_off, seg_len, dst_off), first=first),
             dict(count=n, nseg=seg_len.size, dst_bytes=DST_WIN.size))
    want = S.model_pack(c)["dst"]
    if group == 4:  # the model agrees about the two blocks at the end
        a = int(DST_WIN.near(int(dst_off[-2])))
        assert (want[a:] != CANARY).any() and want[a - 1] == CANARY and want.size - a == int(size[-2])
    far.reset()
    ctx.pack_device(far.src, u64(seg_off), u64(seg_len), u64(first), far.dst, FAR_BYTES, u64(dst_off))
    far.check(want, f"pack group {group}")


@pytest.mark.parametrize("group", range(5))
def test_vlog_frame_far(ctx, far, oracle, group):
    """kvsep_vlog_frame_device with the same placement: headers byte-exact (in group 3 one record's 8-byte header lies
    across 2^32: rec_off = 2^32 - 3), seg_crc and crc_out against the oracle."""
    live = {T32 - 3, T32 + 4099, END} if group == 3 else None
    seg_off, seg_len, first, rec_off, size = placement(group, 8, live=live)
    reach(seg_off, seg_len, first, rec_off, size, 8)
    assert group != 3 or T32 - 3 in [int(x) for x in rec_off]
    n, nseg = rec_off.size, seg_len.size
    c = case("vlog_frame", dict(near_inputs(far, seg_off, seg_len, rec_off), first=first),
             dict(count=n, nseg=nseg, dst_bytes=DST_WIN.size))
    want = S.model_vlog_frame(c)
    far.reset()
    seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
    crc_out = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.vlog_frame_device(far.src, u64(seg_off), u64(seg_len), u64(first), seg_crc, crc_out, far.dst, FAR_BYTES,
                          u64(rec_off), total_bytes=int(seg_len.sum()), max_len=int(seg_len.max()))
    assert np.array_equal(host(seg_crc, np.uint32), want["seg_crc"])
    assert np.array_equal(host(crc_out, np.uint32), want["crc_out"])
    far.check(want["dst"], f"vlog frame group {group}")


@pytest.mark.parametrize("group", range(5))
def test_sst_frame_far(ctx, far, oracle, group):
    """kvsep_sst_frame_device with the same placement (a block is one segment): trailers byte-exact, masked_out
    against the oracle."""
    off, ln, first, blk_off, size = placement(group, 5, one_segment=True)
    reach(off, ln, first, blk_off, size, 5)
    n = blk_off.size
    types = (np.arange(n) % 2).astype(np.uint8)
    near = near_inputs(far, off, ln, blk_off)
    c = case("sst_frame", dict(src=near["src"], off=near["seg_off"], len=ln, types=types, blk_off=near["dst_off"]),
             dict(count=n, dst_bytes=DST_WIN.size))
    want = S.model_sst_frame(c)
    far.reset()
    masked = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.sst_frame_device(far.src, u64(off), u64(ln), dev8(types), masked, far.dst, FAR_BYTES, u64(blk_off),
                         total_bytes=int(ln.sum()), max_len=int(ln.max()))
    assert np.array_equal(host(masked, np.uint32), want["masked_out"])
    far.check(want["dst"], f"sst frame group {group}")


# ------------------------------------------------------------------------------------------------- tier A: layout
def far_blocks(n, top, seed):
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, top + 1, n).astype(np.uint64)
    off = np.array([S_OFF[i % 8] + i // 8 for i in range(n)], np.uint64)
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    return off, ln, keep


def test_offsets_from_far_start_then_pack(ctx, far):
    """kvsep_crc32c_offsets_device from start = 2^32 - 1000 over 300 kept or dropped blocks of up to 64 bytes, its
    dst_off handed to kvsep_crc32c_pack_device as it is: the device-computed offsets cross 2^32 in the middle of a
    1,024-block tile.  (The salvage form itself starts at 0, so the two passes are two calls here.)"""
    n, start = 300, T32 - 1000
    off, ln, keep = far_blocks(n, 64, 5)
    c = case("offsets", dict(near_inputs(far, off, ln, np.zeros(0, np.uint64)), off=None, len=ln),
             dict(count=n, dst_bytes=DST_WIN.size))
    w = S._offsets(c, ln, None, keep, 0, 0, start)
    laid = w["dst_off"][w["dst_off"] != np.uint64(SKIP)]
    assert (laid < T32).any() and (laid > T32).any() and int(w["end"][0]) > T32
    c.inp["off"] = c.inp["seg_off"]
    want = S._salvage(c, dict(dst_off=DST_WIN.near_all(w["dst_off"])), 0)["dst"]
    far.reset()
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    end, nkept = (torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(2))
    ctx.offsets_device(u64(ln), dst_off, end, keep=dev8(keep), start=start, nkept=nkept)
    ctx.pack_device(far.src, u64(off), u64(ln), u64(np.arange(n + 1)), far.dst, FAR_BYTES, dst_off)
    assert np.array_equal(host(dst_off, np.uint64), w["dst_off"])
    assert host(end, np.uint64)[0] == w["end"][0] and host(nkept, np.uint64)[0] == w["nkept"][0]
    far.check(want, "offsets + pack")


def guarded(nbytes, guard=64):
    t = torch.full((nbytes + 2 * guard,), CANARY, dtype=torch.uint8, device=DEV)
    return t, t.data_ptr() + guard, guard


def test_salvage_far_source(ctx, far):
    """kvsep_crc32c_salvage_device over blocks that lie at and across 2^32 in the source.  The form lays out from
    destination offset 0 (the header: "go back to back to dst from offset 0"), so only the source is far."""
    n = 300
    off, ln, keep = far_blocks(n, 64, 6)
    near = near_inputs(far, off, ln, np.zeros(0, np.uint64))
    c = case("salvage", dict(src=near["src"], off=near["seg_off"], len=ln, keep=keep), dict(count=n))
    need = int(ln[keep != 0].sum())
    c.par["dst_bytes"] = need
    w = S.model_salvage(c)
    raw, dst, g = guarded(need)
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    end, nkept = (torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(2))
    ctx.salvage_device(far.src, u64(off), u64(ln), dst, need, dst_off, end, keep=dev8(keep), nkept=nkept, count=n)
    assert np.array_equal(host(dst_off, np.uint64), w["dst_off"])
    assert host(end, np.uint64)[0] == w["end"][0] == need and host(nkept, np.uint64)[0] == w["nkept"][0]
    got = raw.cpu().numpy()
    assert np.array_equal(got[g:g + need], w["dst"]) and (got[:g] == CANARY).all() and (got[g + need:] == CANARY).all()


def test_sst_salvage_far_file(ctx, far, oracle):
    """kvsep_sst_salvage_device over a table image whose 300 blocks of up to 64 bytes, with their trailers, lie across
    2^32 in the source allocation, a tenth of them damaged.  The destination starts at 0, as the form prescribes."""
    n, at = 300, T32 - 9000
    rng = np.random.default_rng(8)
    blocks = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 65, n)]
    img, pos, _ = FB.sst_image(blocks, [int(t) for t in rng.integers(0, 2, n)], oracle)
    img = np.frombuffer(img, np.uint8).copy()
    ln = np.array([len(b) for b in blocks], np.uint64)
    assert at + int(pos[n // 2]) < T32 < at + img.size
    for i in np.flatnonzero(rng.random(n) < 0.1):  # a payload byte, the type byte or a trailer byte
        img[int(pos[i]) + int(rng.integers(0, int(ln[i]) + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    c = case("sst_salvage", dict(src=np.concatenate([img, np.zeros(8, np.uint8)]), off=pos, len=ln),
             dict(count=n, dst_bytes=img.size), out=("ok",))
    w = S.model_sst_salvage(c)
    need = int(w["end"][0])
    assert 0 < int(w["nbad"][0]) < n
    raw, dst, g = guarded(img.size)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    first_bad, nbad, end, nkept = (torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(4))
    try:
        far.src[at:at + img.size] = dev8(img)
        ctx.sst_salvage_device(far.src, u64(pos + np.uint64(at)), u64(ln), out, ok, dst, img.size, dst_off, end,
                               first_bad=first_bad, nbad=nbad, nkept=nkept, count=n, total_bytes=int(ln.sum()),
                               max_len=64)
        torch.cuda.synchronize()
    finally:  # the window holds the splitmix stream again for the tests after this one
        kvsep.fill_splitmix64(far.src.data_ptr() + at, img.size, SEED, at)
        torch.cuda.synchronize()
    assert np.array_equal(host(out, np.uint32), w["out"]) and np.array_equal(host(ok, np.uint8), w["ok"])
    assert np.array_equal(host(dst_off, np.uint64), w["dst_off"])
    for name, t in (("first_bad", first_bad), ("nbad", nbad), ("end", end), ("nkept", nkept)):
        assert host(t, np.uint64)[0] == w[name][0], name
    got = raw.cpu().numpy()
    assert np.array_equal(got[g:g + img.size], w["dst"]) and (got[g:g + need] != CANARY).any()
    assert (got[:g] == CANARY).all() and (got[g + img.size:] == CANARY).all()


@pytest.mark.parametrize("dest_length", [T32 + 12345, 5 * GiB - 7])
def test_log_frame_appends_to_a_far_log(ctx, far, oracle, dest_length):
    """kvsep_log_frame_device appending 70 records of 0..40,000 bytes, read from offsets at and across 2^32, to a log
    whose dest_length is 2^32 + 12,345 (block offset 12,345) and 5 * 2^30 - 7 (block offset 32,761: the call opens
    with a zero trailer).  rec_at and written are relative to the first appended byte; the image is byte-exact against
    the log::Writer model started at that dest_length."""
    n = 70
    rng = np.random.default_rng(dest_length % 1000)
    ln = rng.integers(0, 40001, n).astype(np.uint64)
    ln[[3, 17]] = 0
    ln[5] = FB.BLOCK - FB.HEADER  # fills a block of its own exactly, wherever it starts
    off = np.array([S_OFF[i % 8] for i in range(n)], np.uint64)
    near = np.array([SRC_WIN.near(int(o), int(k)) for o, k in zip(off, ln)], np.uint64)
    phys, _, written = FB.writer([int(x) for x in ln], np.ones(n, np.uint8), dest_length)
    cap = len(phys) + 3
    c = case("log_frame", dict(src=far.src_near, off=near, len=ln),
             dict(count=n, frag_cap=cap, dest_length=dest_length, dst_bytes=written))
    w = S.model_log_frame(c)
    owner = np.searchsorted(w["frag_first"], np.arange(len(phys)), side="right") - 1
    w["frag_off"][:len(phys)] += (off - near)[owner]  # the model's window offsets, back where the records lie
    raw, dst, g = guarded(written)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=DEV)  # noqa: E731
    t = dict(rec_at=i64(n), frag_first=i64(n + 1), frag_off=i64(cap), frag_len=i64(cap), frag_at=i64(cap),
             frag_type=torch.zeros(cap, dtype=torch.uint8, device=DEV),
             frag_crc=torch.zeros(cap, dtype=torch.int32, device=DEV), nfrag=i64(1), written=i64(1))
    ctx.log_frame_device(far.src, u64(off), u64(ln), dest_length, dst, written, t["rec_at"], t["frag_first"],
                         t["frag_off"], t["frag_len"], t["frag_at"], t["frag_type"], t["frag_crc"], t["nfrag"],
                         t["written"], count=n, frag_cap=cap, total_bytes=int(ln.sum()))
    for name, v in t.items():
        assert np.array_equal(host(v, w[name].dtype), w[name]), name
    got = raw.cpu().numpy()
    assert np.array_equal(got[g:g + written], w["dst"])
    assert (got[:g] == CANARY).all() and (got[g + written:] == CANARY).all()


# --------------------------------------------------------------------------------------- tier B: totals that reach 2^32
UNIT = (64 << 20) + 3
UNIT_AT = 7  # the unit's (odd) offset in its allocation
UNIT_SEED = 0xB16B00


class Unit:
    def __init__(self, oracle):
        self.host = splitmix64_bytes(UNIT, UNIT_SEED, 0)
        self.src = torch.empty(UNIT + 32, dtype=torch.uint8, device=DEV)
        kvsep.fill_splitmix64(self.src.data_ptr() + UNIT_AT, UNIT, UNIT_SEED, 0)
        self.dev = self.src[UNIT_AT:UNIT_AT + UNIT]
        self.oracle = oracle
        self.crc = oracle.extend_addr(0, self.host.ctypes.data, UNIT)
        self._chain = {0: 0}

    def chain(self, k):
        """Value(the unit k times): oracle.extend_addr chained, each prefix computed once."""
        have = max(j for j in self._chain if j <= k)
        crc = self._chain[have]
        for j in range(have, k):
            crc = self._chain[j + 1] = self.oracle.extend_addr(crc, self.host.ctypes.data, UNIT)
        return crc

    def value(self, k, cut):
        """Value(the unit k times, then its first `cut` bytes)."""
        return self.oracle.extend_addr(self.chain(k), self.host.ctypes.data, cut)

    def repeats(self, dst, at, k, cut=0):
        """dst[at, ...) holds the unit k times and then its first `cut` bytes (compared on the device)."""
        for j in range(k):
            if not torch.equal(dst[at + j * UNIT:at + (j + 1) * UNIT], self.dev):
                return False
        return cut == 0 or torch.equal(dst[at + k * UNIT:at + k * UNIT + cut], self.dev[:cut])


@pytest.fixture(scope="module")
def unit(oracle):
    u = Unit(oracle)
    yield u
    del u.src, u.dev


def test_pack_one_block_over_4gib(ctx, unit):
    """One plain block of 65 segments of 64 MiB + 3 bytes (the same unit: shared segments are allowed): 65,536 tiles
    whose payload positions pass 2^32, into a destination of 2^32 + 2^27 bytes."""
    k, at, dst_bytes = 65, 4097, T32 + (1 << 27)
    total = k * UNIT
    assert total > T32 and at + total <= dst_bytes
    dst = torch.full((dst_bytes,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.pack_device(unit.src, u64(np.full(k, UNIT_AT)), u64(np.full(k, UNIT)), u64([0, k]), dst, dst_bytes, u64([at]))
    assert unit.repeats(dst, at, k)
    assert is_canary(dst[:at]) and is_canary(dst[at + total:])


@pytest.mark.parametrize("middle", [T32 - 1, T32], ids=["2^32-1", "2^32"])
def test_vlog_frame_auto_at_the_length_word_limit(ctx, unit, oracle, middle):
    """kvsep_vlog_frame_auto_device over a small record, a record of exactly 2^32 - 1 bytes (63 units and a cut one:
    written, with the length word 0xFFFFFFFF, and the record behind it lands past 2^32) or of 2^32 bytes (it and the
    record behind it get KVSEP_OFFSET_SKIP, *end is UINT64_MAX, their bytes stay canary; the first record is still
    written).  crc_out against the oracle chained over the unit."""
    k, cut = middle // UNIT, middle % UNIT
    small = [(UNIT_AT + 5, 100), (UNIT_AT + 1000, 0), (UNIT_AT + UNIT - 50, 50)]
    last = [(UNIT_AT + 333, 1234)]
    seg = small + [(UNIT_AT, UNIT)] * k + [(UNIT_AT, cut)] + last
    seg_off, seg_len = (np.array([s[j] for s in seg], np.uint64) for j in range(2))
    first = np.array([0, 3, 3 + k + 1, 3 + k + 2], np.uint64)
    start = 5
    pay0 = b"".join(unit.host[o - UNIT_AT:o - UNIT_AT + n].tobytes() for o, n in small)
    pay2 = unit.host[333:333 + 1234].tobytes()
    crc = [oracle.extend(0, pay0), unit.value(k, cut), oracle.extend(0, pay2)]
    want_off, want_end, _, _ = FB.ref_offsets(seg_len, first, None, None, 8, 0, start, 0xFFFFFFFF, 3)
    fits = middle < T32
    assert [int(x) for x in want_off] == ([5, 163, 171 + middle] if fits else [5, SKIP, SKIP])
    assert want_end == (171 + middle + 8 + 1234 if fits else U64) and (not fits or int(want_off[2]) > T32)
    dst_bytes = start + 163 - 5 + 8 + T32 + 8 + 1234 + 64
    dst = torch.full((dst_bytes,), CANARY, dtype=torch.uint8, device=DEV)
    nseg = seg_off.size
    seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
    crc_out = torch.zeros(3, dtype=torch.int32, device=DEV)
    rec_off, end = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    ctx.vlog_frame_auto_device(unit.src, u64(seg_off), u64(seg_len), u64(first), seg_crc, crc_out, dst, dst_bytes,
                               rec_off, end, start=start, total_bytes=int(seg_len.sum()), max_len=UNIT)
    assert [int(x) for x in host(crc_out, np.uint32)] == crc
    want_seg = [oracle.extend(0, unit.host[o - UNIT_AT:o - UNIT_AT + n].tobytes()) for o, n in small] + \
        [unit.crc] * k + [unit.value(0, cut), crc[2]]
    assert [int(x) for x in host(seg_crc, np.uint32)] == want_seg
    assert np.array_equal(host(rec_off, np.uint64), want_off) and int(host(end, np.uint64)[0]) == want_end
    header = lambda v, n: struct.pack("<II", S.mask1(v), n & 0xFFFFFFFF)  # noqa: E731
    assert bytes(dst[:163].cpu().numpy()) == bytes([CANARY]) * 5 + header(crc[0], 150) + pay0
    if fits:
        assert header(crc[1], middle)[4:] == b"\xff\xff\xff\xff"
        assert bytes(dst[163:171].cpu().numpy()) == header(crc[1], middle)
        assert unit.repeats(dst, 171, k, cut)
        at2 = 171 + middle
        assert bytes(dst[at2:at2 + 8 + 1234].cpu().numpy()) == header(crc[2], 1234) + pay2
        assert is_canary(dst[at2 + 8 + 1234:])
    else:
        assert is_canary(dst[163:])


def test_salvage_kept_blocks_pass_4gib(ctx, unit):
    """kvsep_crc32c_salvage_device over 70 blocks of the unit with a keep mask: the 66 kept ones pass 2^32 cumulatively,
    so dst_off and *end come from 64-bit sums and the copy writes past 2^32."""
    n = 70
    keep = np.ones(n, np.uint8)
    keep[[0, 13, 40, 69]] = 0
    ln = np.full(n, UNIT, np.uint64)
    want_off, want_end, want_kept, _ = FB.ref_offsets(ln, None, keep, None, 0, 0, 0, U64, n)
    assert want_end == 66 * UNIT > T32 and want_kept == 66
    dst_bytes = want_end + 4096
    dst = torch.full((dst_bytes,), CANARY, dtype=torch.uint8, device=DEV)
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    end, nkept = (torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(2))
    ctx.salvage_device(unit.src, u64(np.full(n, UNIT_AT)), u64(ln), dst, dst_bytes, dst_off, end, keep=dev8(keep),
                       nkept=nkept, count=n)
    assert np.array_equal(host(dst_off, np.uint64), want_off)
    assert int(host(end, np.uint64)[0]) == want_end and int(host(nkept, np.uint64)[0]) == want_kept
    assert unit.repeats(dst, 0, 66) and is_canary(dst[want_end:])


# ------------------------------------------------------------------------------------ tier B: a log image over 4 GiB
PERIOD = 129           # blocks: not a divisor of the 1,024-block tile
LOG_BYTES = T32 + 3 * FB.BLOCK
REPS = LOG_BYTES // (PERIOD * FB.BLOCK)                   # whole periods: 1,016
TAIL_BLOCKS = LOG_BYTES // FB.BLOCK - REPS * PERIOD       # and 11 blocks of one more, the last 3 of them past 2^32
DAMAGED = REPS - 2     # the repetition that is damaged


def period_image(oracle):
    """Records of 5..9 KiB, written by the log::Writer restatement, that fill PERIOD blocks exactly: the last record
    ends with its block, so every chain closes inside the period and a repetition starts like the first."""
    rng = np.random.default_rng(129)
    size, lens, pos, lo, hi = PERIOD * FB.BLOCK, [], 0, 5 << 10, 9 << 10
    one = (lo + 21, hi + 7)  # bytes one record of lo..hi bytes can take, headers and a trailer included
    while pos < size:
        left = size - pos
        k = next((k for k in (left - 7, left - 14, left - 21)
                  if lo <= k <= hi and FB.writer([k], [1], pos)[2] == left), None)
        for _ in range(1000 if k is None else 0):
            k = int(rng.integers(lo, hi + 1))
            rest = left - FB.writer([k], [1], pos)[2]
            if one[0] <= rest <= one[1] or rest >= 2 * one[0]:  # one more record, or two and more, can end the period
                break
        else:
            assert k is not None, "no record length closes the period"
        lens.append(k)
        pos += FB.writer([k], [1], pos)[2]
    data = splitmix64_bytes(sum(lens), 0x10C, 0).tobytes()
    recs, q = [], 0
    for k in lens:
        recs.append(data[q:q + k])
        q += k
    img, phys = FB.log_image(recs, oracle)
    assert len(img) == size
    return img, phys


def log_model(img):
    w = S._log_records(None, len(img) // 4000 + 64, img=img, dst_bytes=len(img))
    w["dst"] = w["dst"][:int(w["end"][0])]
    return w


def stitch(parts, cap):
    """parts = [(model outputs, image offset)] in image order -> the outputs of one call over the whole image."""
    per_rec = ("off", "len", "stored", "type", "ok", "accept", "gap", "frag_off", "frag_len")
    acc = {k: [] for k in per_rec + ("first", "whole", "rec_off", "rec_len")}
    tot = dict(nrec=0, nchain=0, nwhole=0, dropped=0, bad_length=0, end=0)
    for w, shift in parts:
        nrec, nch = int(w["nrec"][0]), int(w["nchain"][0])
        for k in per_rec:
            acc[k].append(w[k][:nrec] + np.uint64(shift) if k in ("off", "frag_off") else w[k][:nrec])
        acc["first"].append(w["first"][:nch] + np.uint64(tot["nrec"]))
        acc["whole"].append(w["whole"][:nch])
        ro = w["rec_off"][:nch]
        acc["rec_off"].append(np.where(ro == np.uint64(SKIP), np.uint64(SKIP), ro + np.uint64(tot["end"])))
        acc["rec_len"].append(w["rec_len"][:nch])
        for k in tot:
            tot[k] += int(w[k][0])
    assert tot["nrec"] <= cap
    pad = {"first": tot["nrec"], "rec_off": SKIP}
    out = {}
    for k, v in acc.items():
        a = np.concatenate(v)
        size = cap + 1 if k == "first" else cap
        out[k] = np.concatenate([a, np.full(size - a.size, pad.get(k, 0), a.dtype)])
    out.update({k: np.array([v], np.uint64) for k, v in tot.items()})
    return out


@pytest.fixture(scope="module")
def big_log(oracle):
    """The image on the device and what log::Reader makes of it: the model over one period, over the damaged repetition
    with its two neighbours, and over the 11 blocks at the end, each shifted to where it lies."""
    period, phys = period_image(oracle)
    pb = len(period)
    win = bytearray(period * 3)
    hurt = []  # (offset in the period, new bytes)
    at = phys[40][0]
    hurt.append((at + 4, b"\xff\xff"))                   # a length past its block: "bad record length"
    at = phys[200][0]
    hurt.append((at, bytes(7)))                          # a zeroed header: the rest of the block is skipped
    at = phys[333][0]
    hurt.append((at, bytes([period[at] ^ 0x04])))        # a bad stored CRC: the rest of the block is dropped
    at = phys[450][0]
    hurt.append((at + 6, b"\x07"))                       # a type byte the checksum does not cover any more
    for o, b in hurt:
        win[pb + o:pb + o + len(b)] = b
    clean, damaged, tail = log_model(period), log_model(bytes(win)), log_model(period[:TAIL_BLOCKS * FB.BLOCK])
    assert int(damaged["dropped"][0]) and int(damaged["bad_length"][0]) and damaged["gap"].any()
    assert int(damaged["nwhole"][0]) < 3 * int(clean["nwhole"][0])
    parts = [(clean, r * pb) for r in range(DAMAGED - 1)] + [(damaged, (DAMAGED - 1) * pb)] + [(tail, REPS * pb)]
    assert DAMAGED + 2 == REPS
    nrec = (DAMAGED - 1) * int(clean["nrec"][0]) + int(damaged["nrec"][0]) + int(tail["nrec"][0])
    cap = nrec + 5
    want = stitch(parts, cap)
    assert int(want["off"][nrec - 1]) > T32 and int(want["nrec"][0]) == nrec
    p = dev8(np.frombuffer(period, np.uint8))
    img = p.repeat(REPS + 1)[:LOG_BYTES]
    for o, b in hurt:
        a = DAMAGED * pb + o
        img[a:a + len(b)] = dev8(np.frombuffer(b, np.uint8))
    torch.cuda.synchronize()
    yield dict(img=img, want=want, cap=cap, clean=clean, damaged=damaged, tail=tail)
    del img


def log_outputs(cap):
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=DEV)  # noqa: E731
    u8 = lambda k: torch.full((k,), 9, dtype=torch.uint8, device=DEV)  # noqa: E731
    return dict(off=i64(cap), len=i64(cap), stored=torch.zeros(cap, dtype=torch.int32, device=DEV), type=u8(cap),
                ok=u8(cap), accept=u8(cap), gap=u8(cap), nrec=i64(1), dropped=i64(1), bad_length=i64(1))


def assert_arrays(t, want, names):
    for name in names:
        w = want[name]
        g = host(t[name], w.dtype)
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{name}[{i}] = {g[i]} want {w[i]} ({int((g != w).sum())} of {w.size} differ)")


READ = ("off", "len", "stored", "type", "ok", "accept", "gap", "nrec", "dropped", "bad_length")


def test_log_read_over_4gib(ctx, big_log):
    """kvsep_log_read_device over an image of 2^32 + 3 * 32,768 bytes (131,075 blocks, about 600 K records; a lane's
    block number times 32,768 passes 2^32 in the last three): off / len / stored / type / ok / accept / gap in full
    against the period's model shifted by rep * 129 * 32,768, the damaged repetition modelled with its neighbours."""
    cap, want = big_log["cap"], big_log["want"]
    ctx.reserve(max(cap, -(-LOG_BYTES // FB.BLOCK)), LOG_BYTES)
    t = log_outputs(cap)
    ctx.log_read_device(big_log["img"], LOG_BYTES, t["off"], t["len"], t["stored"], t["type"], t["ok"], t["accept"],
                        t["nrec"], gap=t["gap"], dropped=t["dropped"], bad_length=t["bad_length"], cap=cap)
    assert_arrays(t, want, READ)


def test_log_records_over_4gib(ctx, big_log):
    """kvsep_log_records_device over the same image: the chains, rec_off / rec_len / *end and the record bytes, compared
    with the model period by period on the device; a destination one byte short leaves the last record unwritten."""
    cap, want = big_log["cap"], big_log["want"]
    ctx.reserve(max(cap, -(-LOG_BYTES // FB.BLOCK)), LOG_BYTES)
    end = int(want["end"][0])
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=DEV)  # noqa: E731

    def run(dst_bytes):
        t = log_outputs(cap)
        t.update(frag_off=i64(cap), frag_len=i64(cap), first=i64(cap + 1),
                 whole=torch.full((cap,), 9, dtype=torch.uint8, device=DEV), nchain=i64(1), rec_off=i64(cap),
                 rec_len=i64(cap), end=i64(1), nwhole=i64(1))
        dst = torch.full((end + 64,), CANARY, dtype=torch.uint8, device=DEV)
        ctx.log_records_device(big_log["img"], LOG_BYTES, t["off"], t["len"], t["stored"], t["type"], t["ok"],
                               t["accept"], t["gap"], t["nrec"], t["frag_off"], t["frag_len"], t["first"], t["whole"],
                               t["nchain"], dst, dst_bytes, t["rec_off"], t["end"], rec_len=t["rec_len"],
                               nwhole=t["nwhole"], dropped=t["dropped"], bad_length=t["bad_length"], cap=cap)
        assert_arrays(t, want, READ + ("frag_off", "frag_len", "first", "whole", "nchain", "nwhole", "rec_off",
                                       "rec_len", "end"))
        return dst

    dst = run(end)
    clean, damaged, tail = (dev8(big_log[k]["dst"]) for k in ("clean", "damaged", "tail"))
    e, k = clean.numel(), DAMAGED - 1
    assert bool((dst[:k * e].view(k, e) == clean).all()), "a clean repetition's records"
    at = k * e
    assert torch.equal(dst[at:at + damaged.numel()], damaged), "the damaged repetition and its neighbours"
    at += damaged.numel()
    assert torch.equal(dst[at:at + tail.numel()], tail) and at + tail.numel() == end
    assert is_canary(dst[end:])
    # one byte short: the last record the reader returns is not written, everything before it is
    nch = int(want["nchain"][0])
    j = max(i for i in range(nch - 40, nch) if want["whole"][i])
    last = int(want["rec_off"][j])
    assert last + int(want["rec_len"][j]) == end
    short = run(end - 1)
    assert torch.equal(short[:last], dst[:last]) and is_canary(short[last:])
