"""The instruments the CRC kernels are judged with, which no other test runs: the streaming-read ceiling kernel
(stream_read_kernel, the denominator of every "fraction of the streaming read" figure), the HIP event timing behind
bench.py's per-kernel times (kvsep_crc32c_ctx_set_timing / _get_timing) and the device data generator
(kvsep_fill_splitmix64_device) at its edges.  Needs a gfx950 device (`-m gpu`).

  * the ceiling kernel reads every 16-byte unit of [src, src + 16 * (nbytes // 16)) once and nothing else: its own
    probe (a thread whose loaded words XOR to 0x9E3779B9 XORs that into *sink) against the statement, one planted word
    per launch;
  * the timing calls count one event pair per call, around the CRC kernel, and the time they report lies between what
    the HBM peak allows and what the host clock saw;
  * the generator equals the splitmix64 recurrence at misaligned destinations, stream offsets past 2^32, the
    grid-stride wrap of both kernels, writes nothing outside [dst, dst + n) and honours its stream argument."""
import time

import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes
from kvsep import workloads as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
MIB = 1 << 20
MAGIC = 0x9E3779B9  # stream_read_kernel's probe word
MAGIC_I32 = MAGIC - (1 << 32)


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


# ------------------------------------------------------------------------------------------------ A1: the read ceiling
def _read_cases(num_cus):
    """[(nbytes, [plants that must leave the magic word], [plants that must leave 0])], plants as byte positions."""
    rng = np.random.default_rng(20240)

    def word_in(lo, hi):  # a 4-byte-aligned position in [lo, hi)
        return int(lo + 4 * rng.integers(0, (hi - lo) // 4))

    cases = [(0, [], [0]), (15, [], [0]), (16, [0], [16])]
    n = MIB - 16  # the tail loop only: no whole chunk
    cases.append((n, [0, 12, n - 16, n - 4], [n, n + 12]))
    # exactly one chunk: one plant in every one of its 1024 rows of 1 KiB (wave = row % 8, rows in flight = row // 8 % 8,
    # round = row // 64), lane and word drawn, the two corners forced
    lanes, words = rng.integers(0, 64, 1024), rng.integers(0, 4, 1024)
    lanes[0], words[0], lanes[1023], words[1023] = 0, 0, 63, 3
    rows = [int(r * 1024 + lanes[r] * 16 + words[r] * 4) for r in range(1024)]
    assert rows[0] == 0 and rows[1023] == MIB - 4
    assert len({(r % 8, r // 8 % 8, r // 64) for r in range(1024)}) == 1024  # every wave, row in flight and round
    cases.append((MIB, rows, [MIB, MIB + 16]))
    cases.append((MIB + 16, [MIB, MIB + 12, word_in(0, MIB)], [MIB + 16]))
    # b: three chunks, a tail of three units and an unread remainder of 5 bytes
    n = 3 * MIB + 48 + 5
    up = (n + 15) // 16 * 16
    inside = [c * MIB + d for c in range(3) for d in (0, MIB - 4)] + [3 * MIB, 3 * MIB + 4, 3 * MIB + 32, 3 * MIB + 44]
    cases.append((n, inside, [3 * MIB + 48, up, up + 16, up + 4080]))
    # c: more chunks than workgroups (the grid is num_cus workgroups: c += gridDim.x), then half a chunk of tail
    nch = num_cus + 3
    tail0, tail_n = nch * MIB, MIB // 2 + 32
    n = tail0 + tail_n
    inside = [word_in(c * MIB, (c + 1) * MIB) for c in (0, num_cus - 1, num_cus, num_cus + 1, nch - 1)]
    inside += [tail0, tail0 + 12, word_in(tail0 + 16, n - 16) // 16 * 16 + 8, n - 16, n - 4]
    cases.append((n, inside, [n, n + 4080]))
    return cases


def test_stream_read_reads_every_unit_once_and_nothing_else():
    """Reference statement: the kernel reads exactly [src, src + 16 * (nbytes // 16)), each 16-byte unit once; the
    last nbytes % 16 bytes and everything from src + nbytes on are not read.  The buffer is zero but for one planted
    u32 0x9E3779B9, so *sink (0 before) ends as the magic word exactly when the plant's unit was loaded an odd number of
    times: once leaves the word, never or twice leaves 0.  One plant per launch, one sink word per launch, one
    read-back per size.  (The tail loop strides by the whole grid's 512 * num_cus threads; a tail is shorter than a
    1 MiB chunk = 65536 units, so from 128 CUs up it never takes a second trip and none is tested.)"""
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = kvsep.Context(0)
    magic = torch.tensor([MAGIC_I32], dtype=torch.int32, device=DEV)
    wrong, n_magic, n_zero = [], 0, 0
    try:
        for nbytes, inside, outside in _read_cases(num_cus):
            buf = torch.zeros((nbytes + 4096 + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            b32 = buf.view(torch.int32)
            plants = [(q, True) for q in inside] + [(q, False) for q in outside]
            # the cases agree with the statement, and every plant lies inside the allocation
            assert all((q < nbytes // 16 * 16) == want and q % 4 == 0 and q + 4 <= nbytes + 4096 for q, want in plants)
            sinks = torch.zeros(len(plants), dtype=torch.int32, device=DEV)
            for i, (q, _) in enumerate(plants):
                b32[q // 4:q // 4 + 1].copy_(magic)
                ctx.stream_read(buf.data_ptr(), nbytes, sinks.data_ptr() + 4 * i)
                b32[q // 4:q // 4 + 1].zero_()
            got = sinks.cpu().numpy().view(np.uint32)
            assert int(buf.view(torch.int64).count_nonzero().item()) == 0  # every plant cleared
            del buf, b32
            for (q, want), g in zip(plants, got):
                if int(g) != (MAGIC if want else 0):
                    wrong.append((nbytes, q, hex(int(g))))
                n_magic += int(g) == MAGIC
                n_zero += int(g) == 0
    finally:
        ctx.close()
    assert not wrong, f"(nbytes, plant, sink) that differ from the statement: {wrong[:12]} ({len(wrong)} in all)"
    # no vacuous pass: the probe was seen to answer both ways -- a word left by every plant inside, 0 by every one outside
    assert n_magic >= 1024 + 28 and n_zero >= 14, (n_magic, n_zero)


# ------------------------------------------------------------------------------------------------ A2: timing
def _uniform(count, length, seed):
    """A packed batch of `count` blocks of `length` bytes of generated data -> (data, off, len, out)."""
    off, ln = W.uniform_layout(count, length)
    d = torch.empty(count * length + 64, dtype=torch.uint8, device=DEV)
    kvsep.fill_splitmix64(d.data_ptr(), count * length, seed, 0)
    return d, dev_u64(off), dev_u64(ln), torch.zeros(count, dtype=torch.int32, device=DEV)


def _host_crcs(count, length, seed):
    buf = splitmix64_bytes(count * length, seed, 0)
    return np.array([kvsep.extend_host(0, buf[i * length:(i + 1) * length]) for i in range(count)], np.uint32)


def test_timing_counts_one_pair_per_call_and_resets():
    """What kvsep_crc32c_ctx_get_timing counts, from the code (launch_batch_body, kvsep_stream_read_device): one event
    pair per call that launches a CRC kernel, recorded around that kernel only -- not around the plan, scan, expand and
    combine kernels of a planned call, the SST prep kernel or the fused compare -- and one per stream_read call.  So:
    batch_device 1 (unsplit or planned), verify_device 1, sst_verify_device 1, stream_read 1; nothing with timing off;
    get_timing hands back the sum and the count and resets both."""
    ctx = kvsep.Context(0)
    try:
        small = _uniform(512, 4096, 11)  # max_len 4096 <= piece: unsplit
        long_ = _uniform(8, 300 * 1024 + 7, 12)  # max_len 0 and blocks longer than the piece: planned
        assert ctx.plan_query(512, 4096, 512 * 4096)[1] == 0
        assert ctx.plan_query(8, 0, 8 * (300 * 1024 + 7))[1] > 0
        sink = torch.zeros(1, dtype=torch.int32, device=DEV)
        fb = torch.zeros(2, dtype=torch.int64, device=DEV)

        def unsplit():
            ctx.batch_device(small[0], small[1], small[2], small[3], max_len=4096, total_bytes=512 * 4096)

        def planned():
            ctx.batch_device(long_[0], long_[1], long_[2], long_[3], max_len=0, total_bytes=8 * (300 * 1024 + 7))

        # off by default: nothing is counted, and a second get_timing at once is (0.0, 0) too
        unsplit()
        planned()
        assert ctx.get_timing() == (0.0, 0)
        assert ctx.get_timing() == (0.0, 0)

        ctx.set_timing(True)
        for _ in range(5):
            unsplit()
        ms, n = ctx.get_timing()
        assert n == 5 and ms > 0.0, (ms, n)
        assert ctx.get_timing() == (0.0, 0)  # reset by the call before
        for _ in range(5):
            planned()
        ms, n = ctx.get_timing()
        assert n == 5 and ms > 0.0, (ms, n)
        torch.cuda.synchronize()
        assert np.array_equal(small[3].cpu().numpy().view(np.uint32), _host_crcs(512, 4096, 11))
        assert np.array_equal(long_[3].cpu().numpy().view(np.uint32), _host_crcs(8, 300 * 1024 + 7, 12))

        unsplit()
        for _ in range(3):
            ctx.stream_read(small[0], 512 * 4096, sink)
        assert ctx.get_timing()[1] == 1 + 3  # three stream_read calls add exactly three

        # the verify form and the SST read check: one pair each (the docstring above)
        exp = torch.zeros(512, dtype=torch.int32, device=DEV)
        ctx.verify_device(small[0], small[1], small[2], exp, small[3], fb[0:1], fb[1:2], max_len=4096,
                          total_bytes=512 * 4096)
        assert ctx.get_timing()[1] == 1
        # blocks of 4091 bytes followed by their 5-byte trailers, in the same data (the verdict is not the point here)
        ln1 = dev_u64(np.full(512, 4091, np.uint64))
        ctx.sst_verify_device(small[0], small[1], ln1, small[3], fb[0:1], fb[1:2], max_len=4091,
                              total_bytes=512 * 4091)
        assert ctx.get_timing()[1] == 1

        ctx.set_timing(False)
        unsplit()
        planned()
        ctx.stream_read(small[0], 512 * 4096, sink)
        assert ctx.get_timing() == (0.0, 0)
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_timing_lies_between_the_hbm_peak_and_the_host_clock():
    """1024 x 1 MiB blocks with max_len = 1 MiB: 1 GiB of payload, four times the 256 MiB Infinity Cache, so every launch
    streams from HBM.  With t = total_ms / launches:
      * t >= payload / 8e12 s: no kernel reads HBM faster than the 8 TB/s peak of the README's roofline -- a pair around
        the wrong (small) kernel, a zero-length pair or a pair in the wrong order reports less;
      * total_ms <= the host's wall clock from just before the first call to just after the synchronize that follows
        the last: the pairs are disjoint intervals inside that region -- a pair spanning several calls, counted per
        call, sums to more.
    Neither bound has a tuned constant, and the second needed no slack for event resolution: on an MI355X the four
    pairs summed to 0.658 ms (164 us each, floor 134 us) inside 0.758 ms of host clock.  What the bounds do not tell
    apart is a pair that closes after the combine kernel instead of before it: that adds a few microseconds to a
    164 us kernel and stays inside both (tried; the launch counts do not change either)."""
    count, length, calls = 1024, MIB, 4
    payload = count * length
    ctx = kvsep.Context(0)
    try:
        d, off, ln, out = _uniform(count, length, 13)

        def call():
            ctx.batch_device(d, off, ln, out, max_len=length, total_bytes=payload)

        call()  # sizes the plan; not timed
        torch.cuda.synchronize()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ctx.set_timing(False)
        total_ms, launches = ctx.get_timing()
        floor_ms = payload / 8e12 * 1e3
        print(f"timing: {launches} launches, {total_ms:.4f} ms in all, {total_ms / max(launches, 1) * 1e3:.1f} us each "
              f"(HBM-peak floor {floor_ms * 1e3:.1f} us), host wall clock {wall_ms:.4f} ms, "
              f"plan {ctx.plan_query(count, length, payload)}")
        assert launches == calls
        assert total_ms / launches >= floor_ms, (total_ms, launches, floor_ms)
        assert total_ms <= wall_ms, (total_ms, wall_ms)
        # the timed calls computed the batch: its first and last blocks against the host leg
        got = out.cpu().numpy().view(np.uint32)
        for i in (0, count - 1):
            assert int(got[i]) == kvsep.extend_host(0, splitmix64_bytes(length, 13, i * length))
    finally:
        ctx.close()


def test_timing_after_an_injected_failure():
    """A call that fails after its CRC kernel (a host-side error return, kvsep_crc32c_ctx_inject_failure) records no
    pair: the two successful calls after it count 2, their events come from the pool the failed call gave its own back
    to, and the context goes on computing right results."""
    ctx = kvsep.Context(0)
    try:
        d, off, ln, out = _uniform(512, 4096, 14)
        want = _host_crcs(512, 4096, 14)
        ctx.set_timing(True)
        ctx.inject_failure()
        with pytest.raises(kvsep.KvsepError, match="injected"):
            ctx.batch_device(d, off, ln, out, max_len=4096, total_bytes=512 * 4096)
        for _ in range(2):
            out.zero_()
            ctx.batch_device(d, off, ln, out, max_len=4096, total_bytes=512 * 4096)
        ms, n = ctx.get_timing()
        assert n == 2 and ms > 0.0, (ms, n)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        # and a planned call that fails the same way
        d2, off2, ln2, out2 = _uniform(8, 300 * 1024 + 7, 15)
        ctx.inject_failure()
        with pytest.raises(kvsep.KvsepError, match="injected"):
            ctx.batch_device(d2, off2, ln2, out2, max_len=0, total_bytes=8 * (300 * 1024 + 7))
        ctx.batch_device(d2, off2, ln2, out2, max_len=0, total_bytes=8 * (300 * 1024 + 7))
        assert ctx.get_timing()[1] == 1
        assert np.array_equal(out2.cpu().numpy().view(np.uint32), _host_crcs(8, 300 * 1024 + 7, 15))
        assert ctx.get_timing() == (0.0, 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ A3: the generator
def _stream_ref(n, seed, so):
    """Bytes [so, so + n) of the splitmix64 stream from the recurrence itself, in numpy uint64: word j =
    mix(seed + (j + 1) * gamma), byte g of the stream = byte g & 7 of word g >> 3 (for any 64-bit offset)."""
    g = np.uint64(so) + np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + ((g >> np.uint64(3)) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> (np.uint64(8) * (g & np.uint64(7)))) & np.uint64(0xFF)).astype(np.uint8)


def _cfg5_offset():
    off, ln = W.cfg3_layout(vlog=True)
    return 7 * int(off[-1] + ln[-1])  # the last slice bench.py --config 5 regenerates: about 448 GiB


def test_generator_reference_is_the_pinned_host_stream():
    """The recurrence written out above equals kvsep.splitmix64_bytes (which the committed goldens pin) where both
    apply, and the config-5 offset is the one the issue of this test names (past 2^32, below 2^40)."""
    for so, n in ((0, 4103), (5, 333), (2**32 - 16, 64), (2**32 + 5, 4103)):
        assert np.array_equal(_stream_ref(n, W.SEED, so), splitmix64_bytes(n, W.SEED, so))
    assert 440 * 2**30 < _cfg5_offset() < 456 * 2**30


GUARD = 64
MISALIGN = (0, 1, 8, 15)
OFFSETS = (0, 1, 8, 15, 16, 2**32 - 16, 2**32 + 5, _cfg5_offset(), 2**40 + 3)
SIZES = (0, 1, 15, 16, 17, 31, 4103)


def _check_fill(host, base, n, ref, what):
    """host = the read-back tensor, [base, base + n) the filled range: equal to ref, every other byte still 0xA5."""
    assert np.array_equal(host[base:base + n], ref), what
    assert (host[:base] == 0xA5).all() and (host[base + n:] == 0xA5).all(), f"{what}: a guard byte was written"


def test_generator_every_alignment_offset_and_size():
    """Every combination of destination misalignment, stream offset and size, each in its own 16-byte-aligned slot of
    one tensor pre-filled with 0xA5, with at least 64 guard bytes on each side: the n bytes equal the stream and no
    byte outside [dst, dst + n) changes.  (Aligned destination and offset % 16 == 0: the 16-byte kernel and, for the
    n % 16 last bytes, a launch of the byte kernel at that offset; everything else: the byte kernel.)"""
    slot = 4352  # >= 64 + 15 + 4103 + 64, a multiple of 16
    cases = [(m, so, n) for m in MISALIGN for so in OFFSETS for n in SIZES]
    t = torch.full((len(cases) * slot,), 0xA5, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    for i, (m, so, n) in enumerate(cases):
        kvsep.fill_splitmix64(t.data_ptr() + i * slot + GUARD + m, n, W.SEED, so)
    host = t.cpu().numpy()
    for i, (m, so, n) in enumerate(cases):
        ref = splitmix64_bytes(n, W.SEED, so) if so < 2**32 - 4103 else _stream_ref(n, W.SEED, so)
        _check_fill(host[i * slot:(i + 1) * slot], GUARD + m, n, ref, f"misalignment {m}, stream offset {so}, n {n}")


@pytest.mark.parametrize("m,so,n", [(0, 2**32 + 16, 8 * MIB + 16 + 3), (1, 2**32 + 5, 600_001)],
                         ids=["fast-kernel", "byte-kernel"])
def test_generator_grid_stride_wrap(m, so, n):
    """More work than one trip of the 2048 x 256 grid: 8 MiB + 16 + 3 bytes for the 16-byte kernel (one unit of a
    second trip, then the 3-byte tail launch, at a stream offset past 2^32), 600,001 bytes for the byte kernel."""
    assert (n // 16 if m == 0 else n) > 2048 * 256
    t = torch.full((GUARD + 16 + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    kvsep.fill_splitmix64(t.data_ptr() + GUARD + m, n, W.SEED, so)
    _check_fill(t.cpu().numpy(), GUARD + m, n, _stream_ref(n, W.SEED, so), f"misalignment {m}, offset {so}, n {n}")


def test_generator_runs_on_the_stream_it_is_given(oracle):
    """A fill on a non-default stream, then a batch_device over the data on the same stream, gives the oracle's CRCs.
    The same stream first fills the whole 256 MiB buffer with 0xA5 and the generated range is its last 4 MiB: a
    generator launched on another stream would run while that fill is still on its way there and be overwritten."""
    n, total = 4 * MIB, 256 * MIB
    off, ln = W.uniform_layout(64, n // 64, first=total - n)
    want = oracle.batch(splitmix64_bytes(n, 21, 0), off - np.uint64(total - n), ln, threads=4)
    buf = torch.empty(total, dtype=torch.uint8, device=DEV)
    doff, dln = dev_u64(off), dev_u64(ln)
    out = torch.zeros(64, dtype=torch.int32, device=DEV)
    ctx = kvsep.Context(0)
    try:
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            buf.fill_(0xA5)
        kvsep.fill_splitmix64(buf.data_ptr() + total - n, n, 21, 0, stream=s)
        ctx.batch_device(buf, doff, dln, out, max_len=n // 64, total_bytes=n, stream=s)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        torch.cuda.synchronize()
    finally:
        ctx.close()
