"""GPU: the SST table reader on the device (kvsep_sst_index_device, kvsep_sst_table_verify_device).

  walk      the device walk equals the host walk element for element, count and status included, on the reference's
            tests/golden/ref_table.sst, on synthetic tables of 0, 1, 64, 65 and 1,025 blocks at restart intervals 1 and
            16 and on damaged index blocks, at cap below, at and above the count;
  table     the table form on all 231 mutants of framing_corpus_sst.json gives the verdicts the reference's reader
            recorded; a wrong magic, n = 47, a handle that leaves the file and a compressed index block give their
            status; canaries around every output stay intact;
  capture   one call captured after reserve, replayed over three mutants uploaded in place;
  salvage   the table form's arrays go to kvsep_sst_salvage_device as they are."""
import json
import os

import numpy as np
import pytest

import framing_corpus as FC
import kvsep
import sst_tables as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 8  # canary elements on each side of every output
C64, C32, C8 = -0x3A3A3A3A3A3A3A3B, -0x3A3A3A3B, 0xC5
NONE = 2 ** 64 - 1


def upload(img):
    return torch.frombuffer(bytearray(bytes(img)), dtype=torch.uint8).to(DEV)


class Outs:
    """Every output of the two forms for `cap` slots, each between GUARD canary elements."""
    SPEC = {"off": (torch.int64, C64, None), "len": (torch.int64, C64, None), "crc": (torch.int32, C32, None),
            "ok": (torch.uint8, C8, None), "bad_idx": (torch.int64, C64, None), "handles": (torch.int64, C64, 4),
            "nblocks": (torch.int64, C64, 1), "first_bad": (torch.int64, C64, 1), "nbad": (torch.int64, C64, 1),
            "status": (torch.int32, C32, 1)}

    def __init__(self, cap):
        self.cap = cap
        self.t = {k: torch.full(((n or cap) + 2 * GUARD,), c, dtype=dt, device=DEV) for k, (dt, c, n) in self.SPEC.items()}

    def p(self, name):
        n = self.SPEC[name][2] or self.cap
        return self.t[name][GUARD:GUARD + n]

    def get(self, name, dtype=None):
        a = self.p(name).cpu().numpy()
        return a.view(dtype) if dtype else a

    def word(self, name):
        return int(self.get(name, np.uint64 if self.SPEC[name][0] is torch.int64 else np.uint32)[0])

    def guards_intact(self):
        for name, (dt, c, n) in self.SPEC.items():
            a = self.t[name].cpu().numpy()
            n = n or self.cap
            assert (a[:GUARD] == c).all() and (a[GUARD + n:] == c).all(), f"a canary around {name} was written"

    def untouched(self, *names):
        for name in names:
            assert (self.t[name].cpu().numpy() == self.SPEC[name][1]).all(), f"{name} was written"


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden_table():
    with open(os.path.join(GOLDEN, "ref_table.sst"), "rb") as f:
        img = f.read()
    with open(os.path.join(GOLDEN, "ref_framing.json")) as f:
        blocks = json.load(f)["sst"]["blocks"]
    return img, blocks


# ------------------------------------------------------------------ the walk alone
def check_walk(ctx, img, index, caps, what):
    """The device walk of the index block `index` = (off, len) of img against the host walk of the same bytes."""
    img = bytes(img)
    d = upload(img)
    handle = torch.tensor(list(index), dtype=torch.int64, device=DEV)
    block = img[index[0]:index[0] + index[1]]
    for cap in caps:
        want_off, want_len, want_n, want_status = kvsep.sst_index_walk(block, cap=cap)
        o = Outs(cap)
        ctx.sst_index_device(d.data_ptr(), len(img), handle, o.p("off"), o.p("len"), o.p("nblocks"), o.p("status"),
                             cap=cap)
        torch.cuda.synchronize()
        assert (o.word("nblocks"), o.word("status")) == (want_n, want_status), (what, cap)
        assert np.array_equal(o.get("off", np.uint64), want_off), (what, cap)
        assert np.array_equal(o.get("len", np.uint64), want_len), (what, cap)
        o.guards_intact()
        o.untouched("crc", "ok", "bad_idx", "handles", "first_bad", "nbad")
    return want_n, want_status


def caps_around(n):
    return sorted({max(n - 1, 0), n, n + 3})


def test_walk_of_the_reference_table(ctx, golden_table):
    img, blocks = golden_table
    ctx.reserve(2048, len(img))
    n, status = check_walk(ctx, img, blocks[53][:2], caps_around(52) + [0], "the reference's table")
    assert (n, status) == (52, kvsep.SST_OK)


@pytest.mark.parametrize("interval", [1, 16])
@pytest.mark.parametrize("nblocks", [0, 1, 64, 65, 1025])
def test_walk_of_synthetic_tables(ctx, nblocks, interval):
    img, off, ln, meta, index = T.build_table(nblocks, interval, seed=nblocks + interval)
    ctx.reserve(max(index[1] // 4, nblocks + 3), img.size)  # cap below the count still walks every run
    n, status = check_walk(ctx, img, index, caps_around(nblocks), f"{nblocks} blocks at interval {interval}")
    assert (n, status) == (nblocks, kvsep.SST_OK)


def test_walk_of_damaged_index_blocks(ctx, golden_table):
    """Two errors (the lower run's wins), a restart array out of order, a restart count the block cannot hold, one the
    reservation cannot hold, and a handle that leaves the image: each as the host walk reports it."""
    img, blocks = golden_table
    ioff, ilen = blocks[53][:2]
    nr = int.from_bytes(img[ioff + ilen - 4:ioff + ilen], "little")
    ro = ioff + ilen - 4 * (1 + nr)
    restart = lambda r: int.from_bytes(img[ro + 4 * r:ro + 4 * r + 4], "little")
    ctx.reserve(2048, len(img))
    hurt = bytearray(img)
    hurt[ioff + restart(30)] = 1  # shared = 1 on a run's first entry
    hurt[ioff + restart(10) + 2] = 0  # no room for a handle in run 10
    assert check_walk(ctx, hurt, (ioff, ilen), [9, 10, 11, 60], "two errors") == (10, kvsep.SST_BAD_HANDLE)
    hurt = bytearray(img)
    hurt[ro + 4 * 7:ro + 4 * 7 + 4] = restart(6).to_bytes(4, "little")
    assert check_walk(ctx, hurt, (ioff, ilen), [60], "restart out of order")[1] == kvsep.SST_BAD_RESTARTS
    hurt = bytearray(img)
    hurt[ioff + ilen - 4:ioff + ilen] = (10 ** 6).to_bytes(4, "little")
    assert check_walk(ctx, hurt, (ioff, ilen), [60], "restart count") == (0, kvsep.SST_BAD_RESTARTS)
    assert check_walk(ctx, img, (ioff, 3), [4], "a block of 3 bytes") == (0, kvsep.SST_BAD_RESTARTS)
    # a handle that leaves the image is not walked: the footer's rule
    d = upload(img)
    for handle in ((ioff, len(img)), (2 ** 63, 2 ** 63), (len(img) - 4, 0)):
        o = Outs(4)
        ctx.sst_index_device(d.data_ptr(), len(img), torch.tensor(np.array(handle, np.uint64).view(np.int64)).to(DEV),
                             o.p("off"), o.p("len"), o.p("nblocks"), o.p("status"), cap=4)
        torch.cuda.synchronize()
        assert (o.word("nblocks"), o.word("status")) == (0, kvsep.SST_BAD_FOOTER)
        assert not o.get("off").any() and not o.get("len").any()
        o.guards_intact()


def test_more_runs_than_the_scratch_holds_stops_the_walk():
    """The restart count is device data: a block with more runs than the scratch was sized for (cap here: nothing is
    reserved) stops with KVSEP_SST_BAD_RESTARTS and lists nothing."""
    img, off, ln, meta, index = T.build_table(300, 1, seed=5)
    c = kvsep.Context(0)
    try:
        d = upload(img)
        o = Outs(40)
        c.sst_index_device(d.data_ptr(), img.size, torch.tensor(list(index), dtype=torch.int64, device=DEV),
                           o.p("off"), o.p("len"), o.p("nblocks"), o.p("status"), cap=40)
        torch.cuda.synchronize()
        assert (o.word("nblocks"), o.word("status")) == (0, kvsep.SST_BAD_RESTARTS)
        assert not o.get("off").any() and not o.get("len").any()
        o.guards_intact()
    finally:
        c.close()


# ------------------------------------------------------------------ the table form
def run_table(ctx, d, n, o, bad_cap=None, max_len_hint=0, stream=None):
    ctx.sst_table_verify_device(d.data_ptr() if hasattr(d, "data_ptr") else d, n, o.p("off"), o.p("len"), o.p("crc"),
                                o.p("ok"), o.p("nblocks"), o.p("handles"), o.p("status"), first_bad=o.p("first_bad"),
                                nbad=o.p("nbad"), bad_idx=o.p("bad_idx"), bad_cap=o.cap if bad_cap is None else bad_cap,
                                cap=o.cap, max_len_hint=max_len_hint, stream=stream)


def check_mutant(o, blocks, bad, what, img):
    """The outputs of the table form on a mutant of the reference's table whose bad blocks (indices into `blocks`: 52
    data blocks, the metaindex block, the index block) the reference's reader recorded as `bad`."""
    cap = o.cap
    handles = [b[:2] for b in blocks]
    assert o.get("handles", np.uint64).tolist() == handles[52] + handles[53], what
    if 53 in bad:  # no handle of an index block that failed its read check is trusted
        assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_INDEX_CHECKSUM, 0), what
        slots, want_bad = handles[52:], [i - 52 for i in bad if i >= 52]
    else:
        assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_OK, 52), what
        slots, want_bad = handles, list(bad)
    pad = cap - len(slots)
    assert o.get("off", np.uint64).tolist() == [h[0] for h in slots] + [0] * pad, what
    assert o.get("len", np.uint64).tolist() == [h[1] for h in slots] + [0] * pad, what
    ok = np.ones(cap, np.uint8)  # padding is a block of length 0 that passes
    ok[want_bad] = 0
    assert np.array_equal(o.get("ok"), ok), what
    assert o.word("nbad") == len(want_bad) and o.word("first_bad") == (want_bad[0] if want_bad else NONE), what
    assert o.get("bad_idx", np.uint64)[:len(want_bad)].tolist() == want_bad, what
    crc = o.get("crc", np.uint32)
    for i in range(len(slots)):
        if ok[i]:  # a block that passes: its CRC is the one its trailer stores
            at = slots[i][0] + slots[i][1] + 1
            assert int(crc[i]) == kvsep.unmask(int.from_bytes(img[at:at + 4], "little")), (what, i)
    assert not crc[len(slots):].any(), what
    o.guards_intact()


def test_table_form_on_the_recorded_corpus(ctx, golden_table):
    """All 231 mutants, at cap = 54 (exact) and 57 (three padding slots) in turn."""
    _, blocks = golden_table
    doc, base = FC.load("sst")
    ctx.reserve(2048, len(base))
    d = upload(base)
    k = 0
    for cls, mutants in doc["classes"].items():
        for m in mutants:
            img = FC.mutate(base, m)
            assert len(img) == len(base)
            d.copy_(upload(img))
            o = Outs(54 if k % 2 else 57)
            run_table(ctx, d, len(img), o, max_len_hint=4300 if k % 3 else 0)
            torch.cuda.synchronize()
            check_mutant(o, blocks, m["bad"], FC.describe(cls, m), img)
            k += 1
    assert k == 231
    assert any(53 in m["bad"] for ms in doc["classes"].values() for m in ms)


def test_table_form_statuses(ctx, golden_table):
    img, blocks = golden_table
    n = len(img)
    ioff, ilen = blocks[53][:2]
    ctx.reserve(2048, n)

    def table(image, cap=57, n_=None):
        d = upload(image)
        o = Outs(cap)
        run_table(ctx, d, len(image) if n_ is None else n_, o)
        torch.cuda.synchronize()
        o.guards_intact()
        return o

    def lists_nothing(o):
        assert o.word("nblocks") == 0 and o.get("handles").tolist() == [0] * 4
        assert not o.get("off").any() and not o.get("len").any() and not o.get("crc").any()
        assert (o.get("ok") == 1).all() and (o.word("nbad"), o.word("first_bad")) == (0, NONE)

    wrong = bytearray(img)
    wrong[-2] ^= 0x20  # a wrong magic
    o = table(wrong)
    assert o.word("status") == kvsep.SST_BAD_FOOTER
    lists_nothing(o)
    o = table(img[-48:], n_=47)  # n = 47: shorter than a footer
    assert o.word("status") == kvsep.SST_BAD_FOOTER
    lists_nothing(o)
    leaves = bytearray(img)
    leaves[-48:] = T.footer(tuple(blocks[52][:2]), (ioff, ilen + 49))  # index_off + index_len + 5 = n + 1
    o = table(leaves)
    assert o.word("status") == kvsep.SST_BAD_FOOTER
    lists_nothing(o)
    # a type byte of 1 on the index block, with the trailer a writer would give it: the checksum passes, the walk is off
    comp = bytearray(img)
    comp[ioff + ilen:ioff + ilen + 5] = T.trailer(img[ioff:ioff + ilen], 1)
    o = table(comp)
    assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_INDEX_COMPRESSED, 0)
    assert o.get("off", np.uint64)[:2].tolist() == [blocks[52][0], ioff] and not o.get("off")[2:].any()
    assert (o.get("ok") == 1).all() and o.word("nbad") == 0
    assert o.get("crc", np.uint32)[1] == kvsep.unmask(int.from_bytes(comp[ioff + ilen + 1:ioff + ilen + 5], "little"))
    comp[ioff + 100] ^= 4  # ... and with a damaged byte the checksum comes first
    o = table(comp)
    assert (o.word("status"), o.word("nbad"), o.word("first_bad")) == (kvsep.SST_INDEX_CHECKSUM, 1, 1)
    # fewer slots than blocks: the first cap - 2 data blocks, then the footer's two; the count stays whole
    o = table(img, cap=12)
    assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_CAP, 52)
    assert o.get("off", np.uint64).tolist() == [b[0] for b in blocks[:10]] + [blocks[52][0], ioff]
    assert (o.get("ok") == 1).all()
    o = table(img, cap=2)
    assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_CAP, 52)
    assert o.get("len", np.uint64).tolist() == [8, ilen] and (o.get("ok") == 1).all()
    # an emitted handle that leaves the image is reported bad and never dereferenced
    keys, handles = T.parse_index(img[ioff:ioff + ilen])
    handles[5] = (2 ** 64 - 2, 7)
    n2 = ioff + len(T.index_block(keys, handles, 1)) + 5 + 48
    handles[3] = (n2 - 4, 0)  # off + len + 5 = n + 1
    blk = T.index_block(keys, handles, 1)
    wild = bytearray(img[:ioff]) + blk + T.trailer(blk) + T.footer(tuple(blocks[52][:2]), (ioff, len(blk)))
    assert len(wild) == n2
    o = table(wild, cap=54)
    assert (o.word("status"), o.word("nblocks")) == (kvsep.SST_OK, 52)
    assert o.get("off", np.uint64)[:6].tolist() == [h[0] for h in handles[:6]]
    assert o.get("bad_idx", np.uint64)[:2].tolist() == [3, 5] and o.word("nbad") == 2
    assert o.get("crc")[3] == 0 and o.get("crc")[5] == 0 and o.get("ok").sum() == 52


def test_synthetic_table_with_many_blocks(ctx):
    """1,025 blocks at restart interval 16 (65 runs of up to 16 entries) through the table form."""
    img, off, ln, meta, index = T.build_table(1025, 16, seed=9)
    ctx.reserve(2048, img.size)
    hurt = img.copy()
    bad = [0, 511, 1024]
    for i in bad:
        hurt[int(off[i]) + 3] ^= 1
    o = Outs(1030)
    run_table(ctx, upload(hurt), hurt.size, o, bad_cap=2, max_len_hint=int(ln.max()))
    torch.cuda.synchronize()
    assert (o.word("status"), o.word("nblocks"), o.word("nbad")) == (kvsep.SST_OK, 1025, 3)
    assert np.array_equal(o.get("off", np.uint64)[:1027], np.concatenate([off, np.array([meta[0], index[0]], np.uint64)]))
    assert np.array_equal(o.get("len", np.uint64)[:1027], np.concatenate([ln, np.array([meta[1], index[1]], np.uint64)]))
    assert np.flatnonzero(o.get("ok") == 0).tolist() == bad
    assert o.get("bad_idx", np.uint64)[:2].tolist() == bad[:2] and o.get("bad_idx")[2] == C64  # bad_cap = 2
    o.guards_intact()


# ------------------------------------------------------------------ capture
def test_captured_table_form_follows_each_replay(golden_table):
    """reserve, one call captured into a graph, replayed over three mutants uploaded in place: each replay gives that
    mutant's verdicts, so no state survives from one replay to the next."""
    _, blocks = golden_table
    doc, base = FC.load("sst")
    mutants = [(cls, m) for cls, ms in doc["classes"].items() for m in ms]
    picks = [next(x for x in mutants if 53 in x[1]["bad"]), next(x for x in mutants if len(x[1]["bad"]) > 1 and
                                                                  53 not in x[1]["bad"]),
             next(x for x in mutants if x[1]["bad"] == [0])]
    c = kvsep.Context(0)
    try:
        n = len(base)
        d = upload(base)
        o = Outs(57)
        c.reserve(max(57, n // 4), n)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run_table(c, d, n, o, stream=torch.cuda.current_stream())
        assert c.capture_sets()[1] == 1
        for cls, m in picks + picks[:1]:
            img = FC.mutate(base, m)
            d.copy_(upload(img))
            g.replay()
            torch.cuda.synchronize()
            check_mutant(o, blocks, m["bad"], "replay of " + FC.describe(cls, m), img)
        # more slots than the reservation: refused at capture, nothing enqueued
        big = Outs(max(57, n // 4) + 1)
        torch.cuda.synchronize()
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                run_table(c, d, n, big, stream=torch.cuda.current_stream())
        del g2
        torch.cuda.synchronize()
        big.untouched(*Outs.SPEC)
        del g
        c.release_captures()
    finally:
        c.close()


# ------------------------------------------------------------------ salvage
def test_table_form_feeds_the_salvage(ctx, golden_table):
    """off / len / crc / ok of the table form go to kvsep_sst_salvage_device with no host step between: the destination
    holds the table's good blocks with their trailers, back to back."""
    img, blocks = golden_table
    n, cap = len(img), 54
    bad = [2, 17, 52]
    hurt = bytearray(img)
    for i in bad:
        hurt[blocks[i][0] + blocks[i][1] // 2] ^= 0x40
    ctx.reserve(2048, n)
    d = upload(hurt)
    o = Outs(cap)
    dst = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst_off = torch.zeros(cap, dtype=torch.int64, device=DEV)
    res = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    run_table(ctx, d, n, o)
    ctx.sst_salvage_device(d.data_ptr(), o.p("off"), o.p("len"), o.p("crc"), o.p("ok"), dst.data_ptr(), n + 256,
                           dst_off, res[0:1], nkept=res[1:2], count=cap, total_bytes=n, max_len=4300)
    torch.cuda.synchronize()
    assert o.word("status") == kvsep.SST_OK and np.flatnonzero(o.get("ok") == 0).tolist() == bad
    want = b"".join(bytes(hurt[b[0]:b[0] + b[1] + 5]) for i, b in enumerate(blocks) if i not in bad)
    end, nkept = res.cpu().numpy().view(np.uint64).tolist()
    assert (end, nkept) == (len(want), 54 - len(bad))
    got = dst.cpu().numpy()
    assert got[:end].tobytes() == want and (got[end:] == 0xA5).all()
