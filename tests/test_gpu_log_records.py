"""Record assembly on the device: kvsep_log_chains_device and kvsep_log_records_device against the host functions
(kvsep_log_walk, the library's host leg for the verdicts, kvsep_log_accept_gaps, kvsep_log_chains) and the recorded
reference -- never against the device path itself.

  chains       the chains pass alone on arrays the test writes, no image: counts around the wave, workgroup and tile
               edges, cap at count - 1, count and count + 3, four distributions, chains that cross a tile edge, with and
               without gap on the LAST, a null gap, no fragment arrays, a caller's own stream; guard elements around
               every output.
  corpus       the composite on every mutant of the recorded log corpus at cap = nrec - 1, nrec and nrec + 3: the bytes
               at dst[rec_off[j], + rec_len[j]) of the whole chains are the records log::Reader returned.
  constructed  65 and 1,030 blocks, intact and damaged, a record of 40 fragments with one MIDDLE broken, the chain-gap
               case across a zeroed block, a dst one byte short, an image at base + 3.
  capture      reserve, then the composite under torch.cuda.graph, replayed over an image rewritten in place."""
import numpy as np
import pytest

import kvsep
import framing_corpus as FC
from framing_builders import BLOCK, FIRST, FULL, LAST, MIDDLE, fnv64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import test_gpu_log_read as LR  # noqa: E402  (the image builders and the guarded reader arrays)

DEV = torch.device("cuda:0")
G, S64, S8 = LR.G, LR.S64, LR.S8
U64 = 0xFFFFFFFFFFFFFFFF
SKIP = U64


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Guarded:
    """A device array of n elements between G guard elements that must stay as they are."""

    def __init__(self, n, dtype):
        self.n, self.sentinel = n, S8 if dtype == torch.uint8 else S64
        self.t = torch.full((n + 2 * G,), self.sentinel, dtype=dtype, device=DEV)

    @property
    def p(self):
        return self.t[G:]

    def get(self, name):
        a = self.t.cpu().numpy()
        assert (a[:G] == self.sentinel).all() and (a[G + self.n:] == self.sentinel).all(), f"guard elements of {name}"
        a = a[G:G + self.n]
        return a.view(np.uint64) if a.dtype == np.int64 else a

    def untouched(self):
        return bool((self.t == self.sentinel).all().item())


class ChainOut:
    def __init__(self, cap, words=6):
        self.cap = cap
        self.first = Guarded(cap + 1, torch.int64)
        self.whole = Guarded(cap, torch.uint8)
        self.frag_off, self.frag_len = Guarded(cap, torch.int64), Guarded(cap, torch.int64)
        self.rec_off, self.rec_len = Guarded(cap, torch.int64), Guarded(cap, torch.int64)
        self.words = torch.full((words,), S64, dtype=torch.int64, device=DEV)  # nrec, nchain, nwhole, end

    def word(self, i):
        return int(self.words[i].item()) & U64


def host_chains(ty, accept, gap, cap):
    """kvsep_log_chains on the first min(count, cap) records, padded as the device form pads."""
    count = min(len(ty), cap)
    first, whole, nchain, nwhole = kvsep.log_chains(ty[:count], accept[:count], None if gap is None else gap[:count])
    f = np.full(cap + 1, count, np.uint64)
    f[:count + 1] = first
    w = np.zeros(cap, np.uint8)
    w[:count] = whole
    return f, w, nchain, nwhole, count


def dev_in(a, cap, dtype, junk):
    """The input array on the device: cap elements, junk past the records (which the pass must not read)."""
    t = torch.full((max(cap, 1),), junk, dtype=dtype, device=DEV)
    k = min(len(a), cap)
    if k:
        t[:k] = torch.from_numpy(np.ascontiguousarray(a[:k]).view(np.int64 if dtype == torch.int64 else np.uint8)).to(DEV)
    return t


def check_chains(ctx, ty, accept, gap, cap, what, frag=True, stream=None):
    n = len(ty)
    off = (np.arange(n, dtype=np.uint64) * 40 + 6)
    ln = (np.arange(n, dtype=np.uint64) * 7 % 33 + 1)
    want_first, want_whole, nchain, nwhole, count = host_chains(ty, accept, gap, cap)
    o = ChainOut(cap)
    o.words[0] = n
    d_ty, d_acc = dev_in(ty, cap, torch.uint8, 0xEE), dev_in(accept, cap, torch.uint8, 0xEE)
    d_gap = None if gap is None else dev_in(gap, cap, torch.uint8, 0xEE)
    d_off, d_len = dev_in(off, cap, torch.int64, -3), dev_in(ln, cap, torch.int64, -3)
    ctx.log_chains_device(d_ty, d_acc, o.words[0:1], o.first.p, o.whole.p, o.words[1:2], gap=d_gap,
                          off=d_off if frag else None, length=d_len if frag else None,
                          frag_off=o.frag_off.p if frag else None, frag_len=o.frag_len.p if frag else None,
                          nwhole=o.words[2:3], cap=cap, stream=stream)
    torch.cuda.synchronize()
    assert (o.word(0), o.word(1), o.word(2)) == (n, nchain, nwhole), f"{what}: words, cap {cap}"
    assert np.array_equal(o.first.get("first"), want_first), f"{what}: first, cap {cap}"
    assert np.array_equal(o.whole.get("whole"), want_whole), f"{what}: whole, cap {cap}"
    if frag:
        fo, fl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        fo[:count], fl[:count] = off[:count] + 1, ln[:count] - 1
        assert np.array_equal(o.frag_off.get("frag_off"), fo) and np.array_equal(o.frag_len.get("frag_len"), fl), what
    else:
        assert o.frag_off.untouched() and o.frag_len.untouched(), what
    assert o.word(3) == S64 & U64


COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100]


def distribution(name, n, rng):
    ty = np.full(n, MIDDLE, np.uint8)
    accept, gap = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    if name == "middle after one first":  # whole tiles of kKeep
        ty[:1] = FIRST
    elif name == "full":
        ty[:] = FULL
    elif name == "rejected":
        accept[:] = 0
    else:  # weighted towards MIDDLE, a gap or a rejection about every 200 records
        ty = rng.choice(np.array([MIDDLE] * 12 + [FIRST, LAST, FULL, 0, 5], np.uint8), n)
        gap = (rng.random(n) < 1 / 400).astype(np.uint8)
        accept = (rng.random(n) >= 1 / 400).astype(np.uint8)
    return ty, accept, gap


@pytest.mark.parametrize("name", ["middle after one first", "full", "rejected", "mix"])
def test_chains_pass_alone(ctx, name):
    rng = np.random.default_rng(20261020)
    for n in COUNTS:
        ty, accept, gap = distribution(name, n, rng)
        for cap in sorted({max(n - 1, 0), n, n + 3}):
            check_chains(ctx, ty, accept, gap, cap, f"{name}, {n} records")


@pytest.mark.parametrize("first_at,last_at", [(1023, 1024), (0, 2048)])
@pytest.mark.parametrize("gap_on_last", [0, 1])
def test_chain_across_a_tile_edge(ctx, first_at, last_at, gap_on_last):
    n = last_at + 30
    ty = np.full(n, FULL, np.uint8)
    ty[first_at], ty[first_at + 1:last_at], ty[last_at] = FIRST, MIDDLE, LAST
    accept, gap = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    gap[last_at] = gap_on_last
    want = host_chains(ty, accept, gap, n)
    j = first_at  # the records before the FIRST are chains of their own
    assert want[0][j] == first_at and want[0][j + 1] == (last_at if gap_on_last else last_at + 1)
    assert want[1][j] == (0 if gap_on_last else 1)
    for cap in (n - 1, n, n + 3, last_at, last_at + 1):
        check_chains(ctx, ty, accept, gap, cap, f"FIRST at {first_at}, LAST at {last_at}, gap {gap_on_last}")


def test_null_gap_no_fragment_arrays_and_a_callers_stream(ctx):
    rng = np.random.default_rng(7)
    ty, accept, gap = distribution("mix", 1300, rng)
    check_chains(ctx, ty, accept, None, 1300, "a null gap")
    check_chains(ctx, ty, accept, gap, 1303, "no fragment arrays", frag=False)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    check_chains(ctx, ty, accept, gap, 1299, "a caller's own stream", stream=s)
    check_chains(ctx, ty[:0], accept[:0], gap[:0], 0, "cap 0")


# ------------------------------------------------------------------ the composite
def host_records(img, cap, full=None):
    """Everything the composite writes, from the host functions: the reader's arrays, the chains, the layout."""
    walk, count, ok, accept, gap, dropped, bad_len = LR.host_expect(img, cap, full)
    off, ln, ty = walk[0][:count], walk[1][:count], walk[3][:count]
    first, whole, nchain, nwhole, _ = host_chains(ty, accept, gap, cap)
    recs, rec_off, rec_len, pos = [], np.full(cap, SKIP, np.uint64), np.zeros(cap, np.uint64), 0
    for j in range(nchain):
        if whole[j]:
            r = b"".join(img[int(off[i]) + 1:int(off[i]) + int(ln[i])] for i in range(int(first[j]), int(first[j + 1])))
            rec_off[j], rec_len[j] = pos, len(r)
            pos += len(r)
            recs.append(r)
    fo, fl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    fo[:count], fl[:count] = off + 1, ln - 1
    return dict(reader=(walk, count, ok, accept, gap, dropped, bad_len), first=first, whole=whole, nchain=nchain,
                nwhole=nwhole, recs=recs, rec_off=rec_off, rec_len=rec_len, end=pos, frag_off=fo, frag_len=fl)


class RecordArrays:
    def __init__(self, cap, dst_bytes):
        self.a = LR.Arrays(cap)
        self.o = ChainOut(cap)
        self.dst_bytes = dst_bytes
        self.dst = torch.full((dst_bytes + 128,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(self, c, base, n, stream=None, rec_len=True):
        a, o = self.a, self.o
        c.log_records_device(base, n, a.p("off"), a.p("len"), a.p("stored"), a.p("type"), a.p("ok"), a.p("accept"),
                             a.p("gap"), a.words[0:1], o.frag_off.p, o.frag_len.p, o.first.p, o.whole.p, o.words[1:2],
                             self.dst[64:], self.dst_bytes, o.rec_off.p, o.words[3:4],
                             rec_len=o.rec_len.p if rec_len else None, nwhole=o.words[2:3], dropped=a.words[1:2],
                             bad_length=a.words[2:3], cap=a.cap, stream=stream)

    def check(self, want, what):
        a, o, cap = self.a, self.o, self.a.cap
        walk, count, ok, accept, gap, dropped, bad_len = want["reader"]
        assert a.word(0) == walk[0].size, f"{what}: nrec, cap {cap}"
        for name, w, dt in (("off", walk[0], np.uint64), ("len", walk[1], np.uint64), ("stored", walk[2], np.uint32),
                            ("type", walk[3], np.uint8), ("ok", ok, np.uint8), ("accept", accept, np.uint8),
                            ("gap", gap, np.uint8)):
            assert np.array_equal(a.get(name, dt), LR.padded(w, cap, dt)), f"{what}: {name}, cap {cap}"
        assert (a.word(1), a.word(2)) == (dropped, bad_len), f"{what}: dropped / bad-length bytes, cap {cap}"
        for name in ("first", "whole", "frag_off", "frag_len", "rec_off", "rec_len"):
            assert np.array_equal(getattr(o, name).get(name), want[name]), f"{what}: {name}, cap {cap}"
        assert (o.word(1), o.word(2), o.word(3)) == (want["nchain"], want["nwhole"], want["end"]), f"{what}: words"
        h = self.dst.cpu().numpy()
        assert (h[:64] == 0xA5).all() and (h[64 + self.dst_bytes:] == 0xA5).all(), f"{what}: bytes around dst"
        body = h[64:64 + self.dst_bytes]
        pos = 0
        for r in want["recs"]:
            if pos + len(r) <= self.dst_bytes:
                assert body[pos:pos + len(r)].tobytes() == r, f"{what}: the record at {pos}, cap {cap}"
            else:  # does not lie inside dst: not written at all
                assert (body[pos:] == 0xA5).all(), f"{what}: a record that does not fit was written"
            pos += len(r)
        assert (body[min(pos, self.dst_bytes):] == 0xA5).all(), f"{what}: dst written at or past *end"


def check_records(ctx, img, what, caps=None, shift=0, stream=None, short=0):
    full = LR.host_full(img)
    nrec = full[0][0].size
    d = LR.upload(img, shift)
    out = None
    for cap in caps if caps is not None else sorted({max(nrec - 1, 0), nrec, nrec + 3}):
        want = host_records(img, cap, full)
        ra = RecordArrays(cap, max(want["end"] - short, 0) if short else want["end"] + 40)
        ra.call(ctx, d[shift:].data_ptr(), len(img), stream=stream)
        torch.cuda.synchronize()
        ra.check(want, what)
        out = want
    assert LR.guards_intact(d, img, shift), f"{what}: the image or the bytes around it changed"
    return out


@pytest.mark.parametrize("cls", FC.classes("log"))
def test_records_on_the_corpus(ctx, cls):
    doc, base = FC.load("log")
    for m in doc["classes"][cls]:
        what = FC.describe(cls, m)
        img = FC.mutate(base, m)
        want = check_records(ctx, img, what)  # the last cap is nrec + 3
        got = [[len(r), fnv64(r)] for r in want["recs"]]
        diff = FC.first_difference(got, FC.want_records(m, doc["intact"]))
        assert diff is None, f"{what}: {diff}"


@pytest.fixture(scope="module")
def img65(oracle):
    return LR.many_blocks(oracle, 65)


def test_65_blocks(ctx, img65):
    want = check_records(ctx, img65, "65 blocks")
    assert want["nwhole"] > 60 and any(len(r) > 2 * 16000 for r in want["recs"])  # FIRST + LAST pairs are joined
    check_records(ctx, LR.flip(LR.flip(img65, 40 * BLOCK + 20), 64 * BLOCK + 9), "65 blocks, two damaged")


def test_1030_blocks(ctx, oracle):
    img = LR.many_blocks(oracle, 1030)
    nrec = kvsep.log_walk(img)[0].size
    assert nrec > 1024  # more than one tile of records
    check_records(ctx, img, "1,030 blocks", caps=[nrec])
    check_records(ctx, LR.flip(LR.flip(img, 1025 * BLOCK + 100), 300 * BLOCK + 9), "1,030 blocks, two damaged",
                  caps=[nrec - 1, nrec + 3])


def test_record_of_40_fragments_with_a_broken_middle(ctx, oracle):
    img = LR.phys(oracle, FULL, LR.pay(30))
    img = LR.fill_block(oracle, img, FIRST, 1)
    for k in range(38):
        img = LR.fill_block(oracle, img, MIDDLE, k + 2)
    img += LR.phys(oracle, LAST, LR.pay(500, 9)) + LR.phys(oracle, FULL, LR.pay(70, 3))
    want = check_records(ctx, img, "a record of 40 fragments")
    assert want["nwhole"] == 3 and len(want["recs"][1]) > 38 * 32000
    want = check_records(ctx, LR.flip(img, 20 * BLOCK + 5000), "a record of 40 fragments, one MIDDLE broken")
    assert [len(r) for r in want["recs"]] == [30, 70]


def test_chain_gap_across_a_zeroed_block_is_not_joined(ctx, oracle):
    img = LR.fill_block(oracle, LR.phys(oracle, FULL, LR.pay(100)), FIRST, 1)  # block k ends with a FIRST
    img += b"\0" * BLOCK  # block k + 1 zeroed
    img += LR.phys(oracle, LAST, LR.pay(300, 2)) + LR.phys(oracle, FULL, LR.pay(40, 3))
    want = check_records(ctx, img, "a FIRST, a zeroed block, the LAST")
    assert [len(r) for r in want["recs"]] == [100, 40] and want["reader"][4].tolist() == [0, 0, 1, 0]


def test_dst_one_byte_short_and_unaligned_image(ctx, img65):
    part = img65[:4 * BLOCK + 900]
    want = check_records(ctx, part, "dst one byte short of *end", short=1, caps=[500])
    assert want["end"] > 0 and want["recs"]
    check_records(ctx, LR.flip(part, BLOCK + 30), "an image at base + 3", shift=3)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    check_records(ctx, part, "a caller's own stream", stream=s, caps=[500])


def test_captured_records_follow_each_replay(img65):
    """reserve, then the composite in one graph; the image is rewritten in place between replays."""
    intact = img65[:9 * BLOCK + 500]
    damaged = LR.flip(intact, 2 * BLOCK + 40)
    at = 4 * BLOCK + 4
    damaged = damaged[:at] + b"\xff\xff" + damaged[at + 2:]
    n, nb = len(intact), 10
    cap = kvsep.log_walk(intact)[0].size + 3
    dst_bytes = host_records(intact, cap)["end"] + 40
    c = kvsep.Context(0)
    try:
        d = LR.upload(intact)
        ra = RecordArrays(cap, dst_bytes)
        c.reserve(max(cap, nb), n)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ra.call(c, d.data_ptr(), n, stream=torch.cuda.current_stream())
        assert c.capture_sets()[1] == 1
        for img in (intact, damaged, intact):
            d[:n] = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
            ra.dst.fill_(0xA5)
            g.replay()
            torch.cuda.synchronize()
            ra.check(host_records(img, cap), "replay")
        assert host_records(damaged, cap)["nwhole"] < host_records(intact, cap)["nwhole"]
        # larger than the reservation: refused at capture, nothing enqueued, the sentinel words untouched
        over = max(cap, nb) + 1
        wide = LR.upload(b"\0" * (over * BLOCK))
        torch.cuda.synchronize()
        for kw in (dict(n=n, cap=over), dict(n=over * BLOCK, cap=cap)):
            big = RecordArrays(kw["cap"], dst_bytes)
            torch.cuda.synchronize()
            with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2):
                    big.call(c, wide.data_ptr(), kw["n"], stream=torch.cuda.current_stream())
            del g2
            torch.cuda.synchronize()
            assert (big.a.words.cpu().numpy() == S64).all() and (big.o.words.cpu().numpy() == S64).all()
            assert big.o.first.untouched() and big.o.rec_off.untouched() and bool((big.dst == 0xA5).all().item())
        del g
        c.release_captures()
    finally:
        c.close()


def test_refusals_leave_everything_untouched(ctx):
    o = ChainOut(4)
    t = torch.zeros(4, dtype=torch.uint8, device=DEV)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null nrec"):
        ctx.log_chains_device(t, t, None, o.first.p, o.whole.p, o.words[1:2], cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null nchain"):
        ctx.log_chains_device(t, t, o.words[0:1], o.first.p, o.whole.p, None, cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*go together"):
        ctx.log_chains_device(t, t, o.words[0:1], o.first.p, o.whole.p, o.words[1:2], off=o.rec_off.p, cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*2\^32"):
        ctx.log_chains_device(t, t, o.words[0:1], o.first.p, o.whole.p, o.words[1:2], cap=1 << 32)
    torch.cuda.synchronize()
    assert (o.words.cpu().numpy() == S64).all() and o.first.untouched() and o.whole.untouched()
