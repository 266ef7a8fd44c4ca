"""GPU: the combine made public -- kvsep_crc32c_concat_device (crc32c_concat_kernel), the gather forms built on it and
one buffer over a group.

  * concat_device against the host fold of kvsep.combine: no payload is involved, so segment lengths go up to
    2^64 - 1.  Runs of 0, 1, 2, 3, the short / long threshold (32) - 1 / 0 / + 1, 63, 64, 65, 129, 1,000 and 4,097
    segments in one batch, empty runs between them, zero-length segments inside them, with and without init.
  * gather_device against the oracle's Extend over the concatenated bytes, one case per route of the segment pass
    (sorted-window, claim, wide, planned with split segments and the piece combine kernel feeding the concat); segments
    lie anywhere in the payload, at every alignment, out of order, overlapping.  seg_crc holds every segment's Value.
  * every segmentation of the same bytes gives what batch_device gives for the whole block.
  * out is written for exactly count elements, seg_crc for exactly nseg, payload and descriptors stay as they were.
  * a reserved gather_device call captured into a graph and replayed with the payload rewritten in between.
  * gather_host and Group.extend_host against the oracle.

Malformed first[] is tested on the CPU only (tests/test_concat_run_cpu.py).  A segment over the 64 MiB staging slot in
gather_host is left out: generating and checking it takes the test past a few seconds, and kvsep_crc32c_batch_host's
own tests (tests/test_gpu_host_pipeline.py) cover that path of the segment pass.  Needs a gfx950 device (`-m gpu`)."""
import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
THRESHOLD = 32  # concat::kShortMax (csrc/concat_run.h): up to here one lane folds the run, above it a wavefront
CANARY, MARGIN = 0xA5, 256


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


def test_threshold_is_the_one_in_the_source():
    import os
    import re
    src = open(os.path.join(os.path.dirname(kvsep.LIB_PATH), "..", "csrc", "concat_run.h")).read()
    assert int(re.search(r"constexpr uint64_t kShortMax = (\d+);", src).group(1)) == THRESHOLD


# ---------------------------------------------------------------- concat_device against the fold of kvsep.combine
@pytest.fixture(scope="module")
def concat_batch():
    rng = np.random.default_rng(20261020)
    runs = []
    for n in (0, 1, 2, 3, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, 63, 64, 65, 129, 1000):
        runs += [n, 0]  # an empty run after each
    runs += [1] * 150 + [0, 0, 5, THRESHOLD + 1, 2, 0, 4097]  # several workgroups; the last block is the longest run
    runs = np.array(runs, np.uint64)
    first = np.concatenate([[0], np.cumsum(runs)]).astype(np.uint64)
    nseg = int(first[-1])
    lens = np.array([0, 1, 4096, 2**32 + 77, 2**61, 2**64 - 1], np.uint64)
    seg_len = lens[rng.integers(0, lens.size, nseg)]  # about one segment in six has length 0
    any_len = rng.integers(0, 2**64, nseg, dtype=np.uint64)  # and one in eight any 64-bit length: many set bits
    pick = rng.integers(0, 8, nseg) == 0
    seg_len[pick] = any_len[pick]
    seg_len[-1] = 2**64 - 1
    seg_crc = rng.integers(0, 2**32, nseg, dtype=np.uint64).astype(np.uint32)
    init = rng.integers(0, 2**32, runs.size, dtype=np.uint64).astype(np.uint32)

    def fold(with_init):
        out = np.zeros(runs.size, np.uint32)
        for i in range(runs.size):
            acc = int(init[i]) if with_init else 0
            for j in range(int(first[i]), int(first[i + 1])):
                acc = kvsep.combine(acc, int(seg_crc[j]), int(seg_len[j]))
            out[i] = acc
        return out

    assert set(lens.tolist()) <= set(seg_len.tolist())
    return dict(runs=runs, first=first, nseg=nseg, seg_len=seg_len, seg_crc=seg_crc, init=init,
                exp={True: fold(True), False: fold(False)})


@pytest.mark.parametrize("with_init", [True, False], ids=["init", "no_init"])
def test_concat_device_is_the_fold_of_combine(ctx, concat_batch, with_init):
    b = concat_batch
    out = torch.full((b["runs"].size,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ctx.concat_device(u32(b["seg_crc"]), u64(b["seg_len"]), u64(b["first"]), out,
                      init=u32(b["init"]) if with_init else None)
    torch.cuda.synchronize()
    got, exp = host32(out), b["exp"][with_init]
    wrong = np.nonzero(got != exp)[0]
    assert wrong.size == 0, (wrong[:8], b["runs"][wrong[:8]])
    # the last block ends on the last segment of the batch, and an empty run gives its init
    assert int(b["first"][-1]) == b["nseg"] and b["runs"][-1] == 4097 and got[-1] == exp[-1]
    empty = np.nonzero(b["runs"] == 0)[0]
    assert np.array_equal(got[empty], b["init"][empty] if with_init else np.zeros(empty.size, np.uint32))


def test_concat_device_count_zero(ctx, concat_batch):
    b = concat_batch
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ctx.concat_device(u32(b["seg_crc"]), u64(b["seg_len"]), u64(b["first"][:1]), out, count=0)
    ctx.concat_device(None, None, u64(np.zeros(3, np.uint64)), out, init=u32([7, 9]), count=2, nseg=0)  # no segments
    torch.cuda.synchronize()
    assert host32(out).tolist() == [7, 9, 0x5A5A5A5A, 0x5A5A5A5A]


# ---------------------------------------------------------------- gather_device against the oracle
PAYLOAD_BYTES = 8 << 20


@pytest.fixture(scope="module")
def payload():
    host = splitmix64_bytes(PAYLOAD_BYTES, 4242, 0)
    d = torch.from_numpy(host).to(DEV)
    return host, d, d.clone()


def make_blocks(rng, nseg, max_per_block):
    """first[] of blocks holding 0 .. max_per_block consecutive segments each, covering all nseg segments."""
    first = [0]
    while first[-1] < nseg:
        first.append(min(nseg, first[-1] + int(rng.integers(0, max_per_block + 1))))
    return np.array(first, np.uint64)


def expected(oracle, host, seg_off, seg_len, first, init):
    """(Extend over each block's concatenated bytes, Value of each segment) by the oracle."""
    cat = np.concatenate([host[int(o):int(o + n)] for o, n in zip(seg_off, seg_len)] + [np.zeros(1, np.uint8)])
    pre = np.concatenate([[0], np.cumsum(seg_len, dtype=np.uint64)]).astype(np.uint64)
    boff, bend = pre[first[:-1].astype(np.int64)], pre[first[1:].astype(np.int64)]
    return (oracle.batch(cat, boff, bend - boff, init, threads=8),
            oracle.batch(host, seg_off, seg_len, threads=8))


def route_case(route, rng):
    """(seg_len, max_len hint, segments per block at most, kernel name) of one route of the segment pass."""
    if route == "sorted":  # >= 8,192 ragged segments of <= 4 KiB
        ln = rng.integers(0, 700, 9000).astype(np.uint64)
        ln[rng.integers(0, 9000, 300)] = rng.integers(3000, 4097, 300)
        ln[:3] = [4096, 0, 1]
        return ln, 4096, 9, "crc32c_narrow_sorted_kernel"
    if route == "claim":  # 32,768 uniform 128-B segments
        return np.full(32768, 128, np.uint64), 128, 70, "crc32c_narrow_claim_kernel"
    if route == "wide":  # unsplit wide segments
        return rng.integers(9000, 30001, 300).astype(np.uint64), 30000, 5, "crc32c_pieces_kernel"
    ln = rng.integers(2049, 9000, 500).astype(np.uint64)  # planned at 1 KiB pieces: every segment is split
    return ln, 0, 40, "crc32c_pieces_kernel"


@pytest.mark.parametrize("route", ["sorted", "claim", "wide", "planned"])
def test_gather_device_matches_the_oracle_on_every_route(oracle, payload, route):
    host, d, clone = payload
    rng = np.random.default_rng({"sorted": 1, "claim": 2, "wide": 3, "planned": 4}[route])
    seg_len, hint, per_block, name = route_case(route, rng)
    nseg = seg_len.size
    seg_off = rng.integers(0, PAYLOAD_BYTES - 30001, nseg).astype(np.uint64)  # anywhere: out of order, overlapping
    seg_off[:16] = 4096 + np.arange(16)  # every start alignment
    first = make_blocks(rng, nseg, per_block)
    count = first.size - 1
    init = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    total = int(seg_len.sum())
    c = kvsep.Context(0)
    try:
        if route == "planned":
            c.set_piece_bytes(1024)
            assert c.plan_query(nseg, hint, total)[1] > nseg  # split segments: the piece combine kernel runs
        assert c.kernel_name(nseg, hint, total) == name
        exp, exp_seg = expected(oracle, host, seg_off, seg_len, first, init)
        seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
        out = torch.zeros(count, dtype=torch.int32, device=DEV)
        c.gather_device(d.data_ptr(), u64(seg_off), u64(seg_len), u64(first), seg_crc, out, init=u32(init),
                        total_bytes=total, max_len=hint)
        torch.cuda.synchronize()
        assert np.array_equal(host32(seg_crc), exp_seg), route
        wrong = np.nonzero(host32(out) != exp)[0]
        assert wrong.size == 0, (route, wrong[:8], np.diff(first.astype(np.int64))[wrong[:8]])
        assert int(np.diff(first.astype(np.int64)).max()) > (THRESHOLD if route in ("claim", "planned") else 1)
        assert torch.equal(d, clone)
    finally:
        c.close()


def test_every_segmentation_gives_the_whole_block(ctx, oracle, payload):
    """Split invariance: one block of 1 MiB + 3 bytes at an odd offset, as one segment, as 4 KiB cuts, as 1,500 random
    cuts, as single bytes around longer cuts with empty segments in between -- and batch_device over the whole block."""
    host, d, _ = payload
    rng = np.random.default_rng(5)
    start, n = 12345, (1 << 20) + 3
    cuts = [
        np.array([0, n]),
        np.concatenate([np.arange(0, n, 4096), [n]]),
        np.concatenate([[0], np.sort(rng.integers(0, n + 1, 1500)), [n]]),
        np.concatenate([np.arange(0, 40), [40, 40, 40, 70000, 70000, n - 1, n, n]]),
        np.concatenate([[0], np.sort(rng.integers(0, n + 1, 31)), [n]]),
    ]
    seg_off = np.concatenate([start + c[:-1] for c in cuts]).astype(np.uint64)
    seg_len = np.concatenate([np.diff(c) for c in cuts]).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum([c.size - 1 for c in cuts])]).astype(np.uint64)
    init = np.full(len(cuts), 0xC0FFEE11, np.uint32)
    whole = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.batch_device(d.data_ptr(), u64([start]), u64([n]), whole, init=u32(init[:1]), total_bytes=n)
    seg_crc = torch.zeros(seg_len.size, dtype=torch.int32, device=DEV)
    out = torch.zeros(len(cuts), dtype=torch.int32, device=DEV)
    ctx.gather_device(d.data_ptr(), u64(seg_off), u64(seg_len), u64(first), seg_crc, out, init=u32(init),
                      total_bytes=int(seg_len.sum()))
    torch.cuda.synchronize()
    want = oracle.extend_addr(0xC0FFEE11, host.ctypes.data + start, n)
    assert host32(whole)[0] == want
    assert host32(out).tolist() == [want] * len(cuts)


# ---------------------------------------------------------------- containment
def carve(spans_bytes):
    """A canary-filled arena with each named array inside it, MARGIN canary bytes around each (test_gpu_containment)."""
    spans, end = {}, 0
    for name, nbytes in spans_bytes.items():
        o = (end + MARGIN + 7) // 8 * 8
        spans[name] = (o, nbytes)
        end = o + nbytes
    return torch.full((end + MARGIN,), CANARY, dtype=torch.uint8, device=DEV), spans


def canaries_intact(arena, spans):
    got = arena.cpu().numpy()
    inside = np.zeros(got.size, bool)
    for o, n in spans.values():
        inside[o:o + n] = True
    return np.nonzero(~inside & (got != CANARY))[0], got


@pytest.mark.parametrize("count_limit", [1, 17, 65, None])
def test_gather_writes_exactly_out_and_seg_crc(ctx, oracle, payload, count_limit):
    host, d, clone = payload
    rng = np.random.default_rng(11)
    seg_len = rng.integers(0, 1500, 3000).astype(np.uint64)
    seg_off = rng.integers(0, PAYLOAD_BYTES - 1500, seg_len.size).astype(np.uint64)
    first = make_blocks(rng, seg_len.size, 2 * THRESHOLD)
    if count_limit is not None:
        first = first[:count_limit + 1]
    count, nseg = first.size - 1, int(first[-1])
    seg_len, seg_off = seg_len[:nseg], seg_off[:nseg]
    init = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    arena, spans = carve({"out": 4 * count, "seg_crc": 4 * nseg})
    desc = [u64(seg_off), u64(seg_len), u64(first), u32(init)]
    keep = [t.clone() for t in desc]
    ctx.gather_device(d.data_ptr(), desc[0], desc[1], desc[2], arena.data_ptr() + spans["seg_crc"][0],
                      arena.data_ptr() + spans["out"][0], init=desc[3], count=count, nseg=nseg,
                      total_bytes=int(seg_len.sum()), max_len=1500)
    torch.cuda.synchronize()
    hit, got = canaries_intact(arena, spans)
    assert hit.size == 0, f"canary bytes written at arena offsets {hit[:8]} (carved: {spans})"
    assert torch.equal(d, clone), "the payload was written"
    assert all(torch.equal(a, b) for a, b in zip(desc, keep)), "a descriptor array was written"
    exp, exp_seg = expected(oracle, host, seg_off, seg_len, first, init)
    o, n = spans["out"]
    assert np.array_equal(got[o:o + n].copy().view(np.uint32), exp)
    o, n = spans["seg_crc"]
    assert np.array_equal(got[o:o + n].copy().view(np.uint32), exp_seg)


# ---------------------------------------------------------------- capture
def test_captured_gather_replays_exactly(oracle):
    rng = np.random.default_rng(13)
    nseg, span = 3000, 2 << 20
    seg_len = rng.integers(0, 9000, nseg).astype(np.uint64)  # max_len unknown (0): planned, the plan is in the capture set
    seg_off = rng.integers(0, span - 9000, nseg).astype(np.uint64)
    first = make_blocks(rng, nseg, 2 * THRESHOLD)
    count, total = first.size - 1, int(seg_len.sum())
    init = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    ctx = kvsep.Context(0)
    try:
        data = torch.empty(span, dtype=torch.uint8, device=DEV)
        d_off, d_len, d_first, d_init = u64(seg_off), u64(seg_len), u64(first), u32(init)
        seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
        out = torch.zeros(count, dtype=torch.int32, device=DEV)
        ctx.reserve(nseg, total)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.gather_device(data.data_ptr(), d_off, d_len, d_first, seg_crc, out, init=d_init, total_bytes=total,
                              max_len=0, stream=torch.cuda.current_stream())
        assert ctx.capture_sets()[1] == 1
        for seed in (101, 202):
            kvsep.fill_splitmix64(data.data_ptr(), span, seed, 0)
            out.zero_()
            seg_crc.zero_()
            g.replay()
            torch.cuda.synchronize()
            exp, exp_seg = expected(oracle, splitmix64_bytes(span, seed, 0), seg_off, seg_len, first, init)
            assert np.array_equal(host32(seg_crc), exp_seg), seed
            assert np.array_equal(host32(out), exp), seed
        del g
        ctx.release_captures()
        assert ctx.capture_sets()[1] == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------- the other forms
def test_gather_host_matches_the_oracle(ctx, oracle):
    rng = np.random.default_rng(17)
    host = splitmix64_bytes(1 << 20, 99, 0)
    seg_len = rng.integers(0, 20000, 400).astype(np.uint64)
    seg_len[[0, 7, 399]] = [0, 1, 0]
    seg_off = rng.integers(0, host.size - 20000, seg_len.size).astype(np.uint64)
    first = make_blocks(rng, seg_len.size, 2 * THRESHOLD)
    init = rng.integers(0, 2**32, first.size - 1, dtype=np.uint64).astype(np.uint32)
    segments = [host[int(o):int(o + n)] for o, n in zip(seg_off, seg_len)]
    exp, _ = expected(oracle, host, seg_off, seg_len, first, init)
    assert np.array_equal(ctx.gather_host(segments, first, init=init), exp)
    exp0, _ = expected(oracle, host, seg_off, seg_len, first, None)
    assert np.array_equal(ctx.gather_host(segments, first), exp0)
    assert ctx.gather_host([], [0, 0, 0], init=[5, 6]).tolist() == [5, 6]


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2", "3"])
def test_group_extend_host_matches_the_oracle(oracle, devices):
    host = splitmix64_bytes((1 << 20) + 3 + 5, 31, 0)
    g = kvsep.Group(devices)
    try:
        for n in (0, 1, 2, 5, (1 << 20) + 3):
            for init in (0, 0x9E3779B9):
                buf = host[5:5 + n]  # an odd start
                assert g.extend_host(init, buf) == oracle.extend(init, buf.tobytes()), (devices, n, init)
    finally:
        g.close()
