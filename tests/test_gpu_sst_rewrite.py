"""GPU: the SST table writer on the device (kvsep_sst_index_keys_device, kvsep_sst_index_build_device,
kvsep_sst_table_finish_device, kvsep_sst_table_rewrite_device).

  identity  the rewrite of tests/golden/ref_table.sst with every block good equals the file byte for byte;
  damaged   mutants of framing_corpus_sst.json (first block bad, last bad, several bad) and a copy with every data block
            bad: the output is the kept blocks with their trailers, sst_tables.index_block over the kept keys and the new
            handles, the metaindex block and the footer; the table verify of the output finds a clean table;
  synthetic tables of 0, 1, 64, 65 and 1,025 blocks under five keep masks; the builder alone over handle values across
            the varint widths and key lengths up to 16,384 at four skews of the position, against the host form, with
            guard bytes around the written range;
  refusals  one byte short, a bad index checksum, a bad footer, restart interval 2: nothing written;
  capture   a reserved rewrite replayed over a damaged and then a repaired source; over its reservation it is refused."""
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
FILL = 0xA5
PAD = 64  # guard bytes on each side of a destination


def upload(img):
    return torch.frombuffer(bytearray(bytes(img)), dtype=torch.uint8).to(DEV)


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).to(DEV)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ref_table.sst"), "rb") as f:
        return f.read()


class Rewrite:
    """Every array of one rewrite with `cap` slots into a destination of dst_bytes between PAD guard bytes."""

    def __init__(self, cap, dst_bytes):
        self.cap, self.dst_bytes = cap, dst_bytes
        z = lambda n, dt=torch.int64: torch.full((n,), -7, dtype=dt, device=DEV)
        self.off, self.len, self.key_off, self.key_len, self.dst_off = (z(cap) for _ in range(5))
        self.crc, self.ok = z(cap, torch.int32), z(cap, torch.uint8)
        self.words = z(8)  # nblocks, nkept, index_len, table_bytes, handles[4]
        self.st = z(2, torch.int32)  # status, wstatus
        self.dst = torch.full((dst_bytes + 2 * PAD,), FILL, dtype=torch.uint8, device=DEV)

    def run(self, ctx, d, n, stream=None, max_len_hint=0):
        w = self.words
        ctx.sst_table_rewrite_device(d.data_ptr(), n, self.dst.data_ptr() + PAD, self.dst_bytes, self.off, self.len,
                                     self.key_off, self.key_len, self.crc, self.ok, self.dst_off, w[0:1], w[4:8],
                                     self.st[0:1], w[2:3], w[3:4], self.st[1:2], nkept=w[1:2], cap=self.cap,
                                     max_len_hint=max_len_hint, stream=stream)

    def result(self):
        torch.cuda.synchronize()
        nblocks, nkept, index_len, table_bytes = u64(self.words)[:4].tolist()
        status, wstatus = self.st.cpu().numpy().view(np.uint32).tolist()
        raw = self.dst.cpu().numpy()
        assert (raw[:PAD] == FILL).all() and (raw[PAD + self.dst_bytes:] == FILL).all(), "a guard byte was written"
        return dict(nblocks=nblocks, nkept=nkept, index_len=index_len, table_bytes=table_bytes, status=status,
                    wstatus=wstatus, out=raw[PAD:PAD + self.dst_bytes])


def expected_rewrite(img):
    """The Python expectation for a source whose footer and index block are good -> (image bytes, new handles)."""
    img = bytes(img)
    (_, _, ioff, ilen), st = kvsep.sst_footer(img)
    assert st == kvsep.SST_OK
    keys, handles = T.parse_index(img[ioff:ioff + ilen])
    bad = set(FC.sst_host_bad(img, [list(h) for h in handles]))
    parts, new, kept_keys, p = [], [], [], 0
    for i, (o, k) in enumerate(handles):
        if i in bad:
            continue
        parts.append(img[o:o + k + 5])
        new.append((p, k))
        kept_keys.append(keys[i])
        p += k + 5
    meta = T.index_block([], [])
    idx = T.index_block(kept_keys, new)
    parts += [meta, T.trailer(meta), idx, T.trailer(idx), T.footer((p, 8), (p + 13, len(idx)))]
    return b"".join(parts), new, len(handles)


def check_rewrite(ctx, src, what, slack=100, verify=True):
    src = bytes(src)
    want, new, total = expected_rewrite(src)
    cap = total + 5
    r = Rewrite(cap, len(want) + slack)
    r.run(ctx, upload(src), len(src))
    g = r.result()
    assert (g["status"], g["wstatus"]) == (kvsep.SST_OK, kvsep.SSTW_OK), what
    assert (g["nblocks"], g["nkept"], g["table_bytes"]) == (total, len(new), len(want)), what
    assert g["out"][:len(want)].tobytes() == want, what
    assert (g["out"][len(want):] == FILL).all(), what
    if verify:  # the output is a table the reader accepts, with the new handles
        cap2 = len(new) + 2
        t = lambda dt: torch.zeros(cap2, dtype=dt, device=DEV)
        off, ln, crc, ok = t(torch.int64), t(torch.int64), t(torch.int32), t(torch.uint8)
        w = torch.zeros(8, dtype=torch.int64, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        ctx.sst_table_verify_device(r.dst.data_ptr() + PAD, len(want), off, ln, crc, ok, w[0:1], w[4:8], st,
                                    first_bad=w[1:2], nbad=w[2:3], cap=cap2)
        torch.cuda.synchronize()
        assert int(st[0]) == kvsep.SST_OK and u64(w)[0] == len(new) and u64(w)[2] == 0, what
        assert list(zip(u64(off)[:len(new)].tolist(), u64(ln)[:len(new)].tolist())) == new, what
    return g


# ------------------------------------------------------------------ the rewrite
def test_rewrite_of_the_reference_table_is_the_identity(ctx, golden):
    ctx.reserve(2048, 2 * len(golden))
    want, _, _ = expected_rewrite(golden)
    assert want == golden  # the precondition test_sst_build_cpu.py asserts on the layout
    g = check_rewrite(ctx, golden, "the reference's table")
    assert g["table_bytes"] == len(golden) and g["out"][:len(golden)].tobytes() == golden


def corpus_picks():
    doc, base = FC.load("sst")
    ms = [(cls, m) for cls, ms in doc["classes"].items() for m in ms
          if m["cut"] is None and not m["append"] and m["bad"] and max(m["bad"]) < 52]
    first = next(x for x in ms if x[1]["bad"] == [0])
    last = next(x for x in ms if 51 in x[1]["bad"])  # (no mutant of the corpus has the last block alone)
    several = next(x for x in ms if len(x[1]["bad"]) > 4)
    return base, [first, last, several]


def test_rewrite_of_damaged_copies(ctx):
    base, picks = corpus_picks()
    ctx.reserve(2048, 2 * len(base))
    for cls, m in picks:
        img = FC.mutate(base, m)
        g = check_rewrite(ctx, img, FC.describe(cls, m))
        assert g["nkept"] == 52 - len(m["bad"])
    # every data block bad (no mutant of the corpus does that): the table of no blocks
    hurt = bytearray(base)
    (_, _, ioff, ilen), _ = kvsep.sst_footer(base)
    _, handles = T.parse_index(base[ioff:ioff + ilen])
    for o, k in handles:
        hurt[o + k // 2] ^= 0x10
    g = check_rewrite(ctx, hurt, "every data block bad")
    assert (g["nkept"], g["table_bytes"]) == (0, 13 + 13 + 48)


MASKS = {
    "none": lambda n: np.zeros(n, bool),
    "all": lambda n: np.ones(n, bool),
    "alternating": lambda n: np.arange(n) % 2 == 1,
    "first": lambda n: np.arange(n) == 0,
    "last": lambda n: np.arange(n) == n - 1,
}


@pytest.mark.parametrize("nblocks", [0, 1, 64, 65, 1025])
def test_rewrite_of_synthetic_tables(ctx, nblocks):
    img, off, ln, meta, index = T.build_table(nblocks, seed=nblocks + 3)
    ctx.reserve(2048, 2 * img.size + 4096)
    for name, mask in MASKS.items():
        hurt = img.copy()
        for i in np.flatnonzero(~mask(nblocks)):
            hurt[int(off[i]) + 1] ^= 0x80
        g = check_rewrite(ctx, hurt, f"{nblocks} blocks, keep {name}", verify=name in ("all", "alternating"))
        assert g["nkept"] == int(mask(nblocks).sum())
    if nblocks:
        assert expected_rewrite(img)[0] == img.tobytes()


# ------------------------------------------------------------------ the builder alone
def builder_case():
    vals = [0, 1]
    for b in range(7, 64, 7):
        vals += [(1 << b) - 1, 1 << b]
    vals += [(1 << 64) - 2]
    klens = [0, 1, 127, 128, kvsep_stage() + 1, 16384, 20, 21]
    src = kvsep.splitmix64_bytes(40000, 5).tobytes()
    n = 3 * len(vals)
    ko, kl, bo, bl = [], [], [], []
    p = 0
    for i in range(n):
        k = klens[i % len(klens)]
        ko.append(p), kl.append(k)
        p = (p + k + i % 16 + 1) % (len(src) - 16400)  # every alignment of the key source
        bo.append(vals[i % len(vals)]), bl.append(vals[(7 * i + 3) % len(vals)])
    keep = np.ones(n, np.uint8)
    keep[5::7] = 0
    bo[11] = kvsep.OFFSET_SKIP
    return src, ko, kl, bo, bl, keep


def kvsep_stage():
    return 4096  # sstw::kStageBytes: a key one byte over it takes the unstaged path


@pytest.mark.parametrize("skew", [0, 1, 15, 16])
def test_builder_against_the_host_form(ctx, skew):
    src, ko, kl, bo, bl, keep = builder_case()
    want, want_len, st = kvsep.sst_index_build(src, ko, kl, bo, bl, keep=keep)
    assert st == kvsep.SSTW_OK and len(want) == want_len + 5
    ctx.reserve(2048, 1 << 20)
    d = upload(src)
    room = skew + len(want)
    dst = torch.full((room + 2 * PAD,), FILL, dtype=torch.uint8, device=DEV)
    assert (dst.data_ptr() + PAD) % 16 == 0
    at = dev64([skew])
    res = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)

    def run(dst_bytes, k=torch.from_numpy(keep).to(DEV)):
        ctx.sst_index_build_device(d.data_ptr(), dev64(ko), dev64(kl), dev64(bo), dev64(bl), dst.data_ptr() + PAD,
                                   dst_bytes, at, res[0:1], status, keep=k)
        torch.cuda.synchronize()
        return dst.cpu().numpy(), int(u64(res)[0]), int(status[0])

    got, out_len, st = run(room - 1)  # one byte short: nothing written, the needed length reported
    assert (st, out_len) == (kvsep.SSTW_NO_ROOM, want_len) and (got == FILL).all()
    got, out_len, st = run(room)
    assert (st, out_len) == (kvsep.SSTW_OK, want_len)
    assert got[PAD + skew:PAD + room].tobytes() == want
    assert (got[:PAD + skew] == FILL).all() and (got[PAD + room:] == FILL).all()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1024, 1025])
def test_builder_counts_and_finish(ctx, count):
    """Row and tile edges of the entry count, through the table form: metaindex block, index block, footer."""
    keys = [T.key_of(i) for i in range(count)]
    src = b"".join(keys)
    kl = [len(k) for k in keys]
    ko = np.concatenate([[0], np.cumsum(kl)[:-1]]).astype(np.uint64) if count else []
    bo = [4101 * i for i in range(count)]
    bl = [4096 + i % 3 for i in range(count)]
    keep = (np.arange(count) % 3 != 1).astype(np.uint8)
    kept = np.flatnonzero(keep)
    idx = T.index_block([keys[i] for i in kept], [(bo[i], bl[i]) for i in kept])
    meta = T.index_block([], [])
    end = 1003
    want = meta + T.trailer(meta) + idx + T.trailer(idx) + T.footer((end, 8), (end + 13, len(idx)))
    ctx.reserve(2048, 1 << 20)
    d = upload(src if count else b"\0")
    dst = torch.full((end + len(want) + PAD,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    for dst_bytes, ok in ((end + len(want) - 1, False), (end + len(want), True)):
        ctx.sst_table_finish_device(d.data_ptr(), dev64(ko), dev64(kl), dev64(bo), dev64(bl), dst.data_ptr(),
                                    dst_bytes, dev64([end]), res[0:1], res[1:2], status,
                                    keep=torch.from_numpy(keep).to(DEV), count=count)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        if not ok:
            assert int(status[0]) == kvsep.SSTW_NO_ROOM and u64(res).tolist() == [len(idx), 0] and (got == FILL).all()
            continue
        assert int(status[0]) == kvsep.SSTW_OK and u64(res).tolist() == [len(idx), end + len(want)]
        assert got[end:end + len(want)].tobytes() == want
        assert (got[:end] == FILL).all() and (got[end + len(want):] == FILL).all()


# ------------------------------------------------------------------ refusals
def test_rewrite_refusals(ctx, golden):
    n = len(golden)
    ctx.reserve(2048, 2 * n)
    (moff, _, ioff, ilen), _ = kvsep.sst_footer(golden)

    def nothing(src, status, what):
        r = Rewrite(57, n + 100)
        r.run(ctx, upload(src), len(src))
        g = r.result()
        assert (g["status"], g["wstatus"], g["table_bytes"]) == (status, kvsep.SSTW_SOURCE, 0), what
        assert (g["out"] == FILL).all(), what

    bad = bytearray(golden)
    bad[ioff + 40] ^= 2
    nothing(bad, kvsep.SST_INDEX_CHECKSUM, "an index block with a bad checksum")
    bad = bytearray(golden)
    bad[-3] ^= 1
    nothing(bad, kvsep.SST_BAD_FOOTER, "a bad footer")
    img, *_ = T.build_table(9, interval=2)
    nothing(img.tobytes(), kvsep.SST_SHARED_KEY, "an index block at restart interval 2")
    # one byte short: the data blocks are the salvage's, the index block and the footer are not written
    r = Rewrite(57, n - 1)
    r.run(ctx, upload(golden), n)
    g = r.result()
    assert (g["status"], g["wstatus"], g["table_bytes"], g["index_len"]) == (kvsep.SST_OK, kvsep.SSTW_NO_ROOM, 0, ilen)
    assert g["out"][:moff].tobytes() == golden[:moff] and (g["out"][moff:] == FILL).all()


# ------------------------------------------------------------------ capture
def test_captured_rewrite_follows_each_replay(golden):
    n = len(golden)
    hurt = bytearray(golden)
    (_, _, ioff, ilen), _ = kvsep.sst_footer(golden)
    _, handles = T.parse_index(golden[ioff:ioff + ilen])
    for i in (0, 20, 51):
        hurt[handles[i][0] + 9] ^= 0x04
    c = kvsep.Context(0)
    try:
        c.reserve(max(57, n // 4), 2 * n + 200)
        d = upload(hurt)
        r = Rewrite(57, n + 100)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            r.run(c, d, n, stream=torch.cuda.current_stream())
        assert c.capture_sets()[1] == 1
        for src in (bytes(hurt), golden, bytes(hurt)):  # damaged, repaired, damaged again
            d.copy_(upload(src))
            r.dst.fill_(FILL)
            g.replay()
            got = r.result()
            want, new, _ = expected_rewrite(src)
            assert (got["status"], got["wstatus"], got["nkept"], got["table_bytes"]) == (0, 0, len(new), len(want))
            assert got["out"][:len(want)].tobytes() == want and (got["out"][len(want):] == FILL).all()
        # more slots than the reservation: refused at capture, nothing enqueued
        big = Rewrite(max(57, n // 4) + 1, n + 100)
        torch.cuda.synchronize()
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                big.run(c, d, n, stream=torch.cuda.current_stream())
        del g2
        torch.cuda.synchronize()
        assert (big.result()["out"] == FILL).all() and int(big.st[1]) == -7
        del g
        c.release_captures()
        r2 = Rewrite(57, n + 100)  # and an eager call works after the release
        r2.run(c, upload(golden), n)
        assert r2.result()["out"][:n].tobytes() == golden
    finally:
        c.close()


def test_keys_walk_on_the_device(ctx, golden):
    n = len(golden)
    ctx.reserve(2048, n)
    (_, _, ioff, ilen), _ = kvsep.sst_footer(golden)
    block = golden[ioff:ioff + ilen]
    d = upload(golden)
    for cap in (0, 51, 52, 55):
        want = kvsep.sst_index_keys(block, cap=cap)
        t = [torch.full((cap + 2,), -7, dtype=torch.int64, device=DEV) for _ in range(4)]
        nb = torch.zeros(1, dtype=torch.int64, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        ctx.sst_index_keys_device(d.data_ptr(), n, dev64([ioff, ilen]), t[0][1:], t[1][1:], t[2][1:], t[3][1:], nb, st,
                                  cap=cap)
        torch.cuda.synchronize()
        assert (int(nb[0]), int(st[0])) == want[4:]
        m = min(cap, 52)
        for k in range(4):
            a = u64(t[k])
            shift = ioff if k == 2 else 0  # device key offsets are image-relative
            assert np.array_equal(a[1:1 + m], want[k][:m] + np.uint64(shift)) and not a[1 + m:1 + cap].any()
            assert a[0] == np.uint64(-7 & (2 ** 64 - 1)) and a[1 + cap] == a[0]
    img, *_, index = T.build_table(9, interval=2)
    t = [torch.zeros(9, dtype=torch.int64, device=DEV) for _ in range(4)]
    nb = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.sst_index_keys_device(upload(img).data_ptr(), img.size, dev64(list(index)), *t, nb, st)
    torch.cuda.synchronize()
    assert (int(nb[0]), int(st[0])) == (1, kvsep.SST_SHARED_KEY)
