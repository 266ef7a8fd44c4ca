"""GPU: the list forms of the verify calls -- WHICH blocks mismatch, built on the device.

kvsep_crc32c_verify_list_device / kvsep_sst_verify_list_device / _host / kvsep_log_verify_device /
kvsep_crc32c_group_verify_list_device (include/kvsep_crc32c.h): after the verify call, bad_idx[0, min(nbad, bad_cap))
holds the mismatching block indices in ascending order and ok[0, count) one verdict byte per block; nothing else is
written.  Blocks here are 0..300 bytes at odd offsets of a 1 MiB pool, so payloads are tiny and the counts can sit on
every edge of the compaction: the 64-lane row, the 256-block wave, the 1,024-block tile, many tiles.  Ground truth is
np.nonzero(Mask(oracle CRC) != stored).  Both arrays are allocated between canary words, and bad_idx is pre-filled:
past the list it must be unchanged."""
import json
import os
import sys

import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import framing_builders as FB  # noqa: E402

DEV = torch.device("cuda:0")
NONE = 2**64 - 1
POOL = 1 << 20
TILE = 1024                      # kListTile (csrc/crc32c_verdicts.inc)
GUARD = 8                        # canary words on each side of bad_idx, 8 x GUARD canary bytes on each side of ok
CANARY = 0x5CA1AB1E0DDBA11       # canary word
FILL = 0x0F0F0F0F0F0F0F0F        # what bad_idx holds before the call
OK_CANARY, OK_FILL = 0xA5, 0x77
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001]
PATTERNS = ["none", "all", "first", "last", "every7", "half"]


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


@pytest.fixture(scope="module")
def pool():
    host = splitmix64_bytes(POOL, 0x115700, 0)
    return host, torch.from_numpy(host).to(DEV)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Batch:
    """`count` blocks of 0..300 bytes at odd pool offsets (plus `long_blocks` of 5 KiB), with their oracle CRCs."""

    def __init__(self, pool, oracle, count, seed, long_blocks=0):
        host, self.data = pool
        rng = np.random.default_rng(seed)
        self.n = count
        self.ln = rng.integers(0, 301, count).astype(np.uint64)
        if long_blocks:
            self.ln[rng.choice(count, long_blocks, replace=False)] = 5 * 1024
        self.off = rng.integers(0, (POOL - 6 * 1024) // 2, count).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        self.total = int(self.ln.sum())
        self.max_len = int(self.ln.max()) if count else 0
        self.crc = oracle.batch(host, self.off, self.ln, threads=16) if count else np.zeros(0, np.uint32)
        if count:
            self.d_off, self.d_len = i64(self.off), i64(self.ln)
        else:  # the arrays of an empty batch are still real device pointers (run_list passes count = 0)
            self.d_off, self.d_len = i64(np.zeros(1, np.uint64)), i64(np.zeros(1, np.uint64))

    def stored(self, pattern, seed=5):
        """The stored words with the pattern's blocks made wrong."""
        w = mask(self.crc)
        n = self.n
        bad = np.zeros(n, bool)
        if n:
            if pattern == "all":
                bad[:] = True
            elif pattern == "first":
                bad[0] = True
            elif pattern == "last":
                bad[-1] = True
            elif pattern == "every7":
                bad[::7] = True
            elif pattern == "half":
                bad = np.random.default_rng(seed).random(n) < 0.5
        w[bad] ^= np.uint32(0x00010000)
        return w


_BATCHES = {}


def batch_of(pool, oracle, count):
    if count not in _BATCHES:
        _BATCHES[count] = Batch(pool, oracle, count, 100 + count)
    return _BATCHES[count]


class Guarded:
    """bad_idx[bad_cap] and ok[count] on the device, each between canaries, pre-filled."""

    def __init__(self, bad_cap, count):
        self.bad_cap, self.count = bad_cap, count
        self.idx_all = torch.full((bad_cap + 2 * GUARD,), CANARY, dtype=torch.int64, device=DEV)
        self.idx_all[GUARD:GUARD + bad_cap] = FILL
        self.ok_all = torch.full((count + 16 * GUARD,), OK_CANARY, dtype=torch.uint8, device=DEV)
        self.ok_all[8 * GUARD:8 * GUARD + count] = OK_FILL

    @property
    def bad_idx(self):
        return self.idx_all.data_ptr() + 8 * GUARD

    @property
    def ok(self):
        return self.ok_all.data_ptr() + 8 * GUARD

    def check(self, truth, with_ok, tag):
        """Canaries intact; the list is truth[:bad_cap] and the rest of bad_idx untouched; ok as asked for."""
        idx = self.idx_all.cpu().numpy().view(np.uint64)
        assert np.all(idx[:GUARD] == CANARY) and np.all(idx[GUARD + self.bad_cap:] == CANARY), (tag, "bad_idx canary")
        body = idx[GUARD:GUARD + self.bad_cap]
        k = min(truth.size, self.bad_cap)
        assert np.array_equal(body[:k], truth[:k].astype(np.uint64)), (tag, body[:8], truth[:8])
        assert np.all(body[k:] == FILL), (tag, "bad_idx written past the list")
        okb = self.ok_all.cpu().numpy()
        assert np.all(okb[:8 * GUARD] == OK_CANARY) and np.all(okb[8 * GUARD + self.count:] == OK_CANARY), \
            (tag, "ok canary")
        body = okb[8 * GUARD:8 * GUARD + self.count]
        if with_ok:
            want = np.ones(self.count, np.uint8)
            want[truth] = 0
            assert np.array_equal(body, want), (tag, np.flatnonzero(body != want)[:8])
        else:
            assert np.all(body == OK_FILL), (tag, "ok written without being asked for")


def run_list(ctx, b, stored, bad_cap, with_ok, tag, max_len=None, null_idx=False):
    """One verify_list_device call on the batch, every output checked against the oracle.  -> (first_bad, nbad)"""
    truth = np.flatnonzero(mask(b.crc) != stored)
    g = Guarded(bad_cap, b.n)
    out = torch.zeros(max(b.n, 1), dtype=torch.int32, device=DEV)
    fb = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    nb = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    d_stored = i32(stored) if b.n else torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.verify_list_device(b.data.data_ptr(), b.d_off, b.d_len, d_stored, out, fb, nb,
                           bad_idx=None if null_idx else g.bad_idx, bad_cap=bad_cap, ok=g.ok if with_ok else None,
                           count=b.n, total_bytes=b.total, max_len=b.max_len if max_len is None else max_len)
    torch.cuda.synchronize()
    got = (int(fb.item()) & NONE, int(nb.item()))
    assert got == (int(truth[0]) if truth.size else NONE, truth.size), (tag, got, truth[:8])
    assert np.array_equal(u32(out)[:b.n], b.crc), tag
    g.check(truth, with_ok, tag)
    return got


@pytest.mark.parametrize("count", COUNTS)
def test_counts_and_patterns(count, ctx, pool, oracle):
    """Every count at a row, wave and tile edge and many tiles, under every pattern, with and without ok."""
    b = batch_of(pool, oracle, count)
    for pattern in PATTERNS:
        stored = b.stored(pattern)
        for with_ok in (True, False):
            run_list(ctx, b, stored, count, with_ok, (count, pattern, with_ok))


@pytest.mark.parametrize("pattern", ["half", "every7", "all"])
def test_bad_cap_cuts_the_list(pattern, ctx, pool, oracle):
    """bad_cap 0, 1, nbad - 1, nbad, nbad + 1, count: the list is the first bad_cap entries, *nbad the full count."""
    b = batch_of(pool, oracle, 2 * TILE + 500)
    stored = b.stored(pattern)
    nbad = int((mask(b.crc) != stored).sum())
    assert 1 < nbad
    for cap in sorted({0, 1, nbad - 1, nbad, min(nbad + 1, b.n), b.n}):
        for with_ok in (False, True):
            assert run_list(ctx, b, stored, cap, with_ok, (pattern, cap, with_ok))[1] == nbad
    run_list(ctx, b, stored, 0, True, (pattern, "null bad_idx"), null_idx=True)  # NULL is allowed with bad_cap 0
    run_list(ctx, b, stored, 0, False, (pattern, "nothing asked for"), null_idx=True)


ROUTES = {  # route -> (set_kernel, piece bytes, 5 KiB blocks, max_len hint (None: the batch's), kernel name)
    "narrow": ("narrow16", None, 0, None, "crc32c_narrow_kernel"),
    "claim": ("claim", None, 0, None, "crc32c_narrow_claim_kernel"),
    "sorted": ("sorted", None, 0, None, "crc32c_narrow_sorted_kernel"),
    "wide": ("wide", None, 0, None, "crc32c_pieces_kernel"),
    "planned": ("auto", 1024, 5, 0, "crc32c_pieces_kernel"),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_feeds_the_list_and_agrees_with_verify_device(route, pool, oracle):
    """The list pass reads what the CRC kernels (and the combine kernel of split blocks) wrote: on every route the
    list is the oracle's, and first_bad, nbad and out[] are what verify_device gives on the same batch."""
    kernel, piece, long_blocks, hint, name = ROUTES[route]
    b = Batch(pool, oracle, 3 * TILE + 77, 900 + len(route), long_blocks=long_blocks)
    hint = b.max_len if hint is None else hint
    c = kvsep.Context(0)
    try:
        c.set_kernel(kernel)
        if piece:
            c.set_piece_bytes(piece)
        assert c.kernel_name(b.n, hint, b.total) == name
        assert (c.plan_query(b.n, hint, b.total)[1] > 0) == (route == "planned")
        for pattern in ("half", "none", "last"):
            stored = b.stored(pattern)
            if route == "planned":  # the split blocks among the bad ones
                stored[b.ln == 5 * 1024] ^= np.uint32(4)
            got = run_list(c, b, stored, b.n, True, (route, pattern), max_len=hint)
            out = torch.zeros(b.n, dtype=torch.int32, device=DEV)
            fb = torch.zeros(1, dtype=torch.int64, device=DEV)
            nb = torch.zeros(1, dtype=torch.int64, device=DEV)
            c.verify_device(b.data.data_ptr(), b.d_off, b.d_len, i32(stored), out, fb, nb, total_bytes=b.total,
                            max_len=hint)
            torch.cuda.synchronize()
            assert (int(fb.item()) & NONE, int(nb.item())) == got, (route, pattern)
            assert np.array_equal(u32(out), b.crc)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ SST
def test_sst_list_forms_name_the_damaged_blocks(ctx):
    """The reference TableBuilder's SST: one byte flipped in three blocks -- the first and the last handle among them --
    and the device and host list forms return exactly those three, ascending; the untouched image an empty list."""
    with open(os.path.join(HERE, "golden", "ref_framing.json")) as f:
        blocks = json.load(f)["sst"]["blocks"]
    with open(os.path.join(HERE, "golden", "ref_table.sst"), "rb") as f:
        sst = f.read()
    off = np.array([x[0] for x in blocks], np.uint64)
    ln = np.array([x[1] for x in blocks], np.uint64)
    n = off.size
    assert n >= 4
    damaged = [0, n // 2, n - 1]
    img = bytearray(sst)
    img[int(off[0]) + int(ln[0]) // 2] ^= 0x20       # a payload byte
    img[int(off[n // 2] + ln[n // 2])] ^= 0x01       # a type byte
    img[int(off[n - 1] + ln[n - 1]) + 2] ^= 0x80     # a byte of the stored word
    for image, want in ((bytes(sst), []), (bytes(img), damaged)):
        d = torch.frombuffer(bytearray(image), dtype=torch.uint8).to(DEV)
        g = Guarded(n, n)
        out = torch.zeros(n, dtype=torch.int32, device=DEV)
        fb = torch.zeros(1, dtype=torch.int64, device=DEV)
        nb = torch.zeros(1, dtype=torch.int64, device=DEV)
        ctx.sst_verify_list_device(d.data_ptr(), i64(off), i64(ln), out, fb, nb, bad_idx=g.bad_idx, bad_cap=n,
                                   ok=g.ok, max_len=int(ln.max()))
        torch.cuda.synchronize()
        assert (int(fb.item()), int(nb.item())) == (want[0] if want else -1, len(want))
        g.check(np.array(want, np.int64), True, ("sst device", len(want)))
        h_out, h_fb, h_nb, h_bad = ctx.sst_verify_list(image, off, ln)
        assert (h_fb, h_nb, h_bad.tolist()) == (want[0] if want else -1, len(want), want)
        assert np.array_equal(h_out, u32(out))
        assert np.array_equal(h_out, ctx.sst_verify(image, off, ln)[0])
        if want:  # the host form's cap
            _, _, nb2, bad2 = ctx.sst_verify_list(image, off, ln, bad_cap=2)
            assert nb2 == 3 and bad2.tolist() == want[:2]


def test_sst_forms_post_the_verdict_of_no_handles_on_a_fresh_context():
    """count == 0 on a context whose scratch never held SST arrays (found by the forms soak, lists/20261021/1): the
    read check, its list form and the salvage write *first_bad = UINT64_MAX and *nbad = 0 as the verify form does; they
    used to leave both words as they were there, and to write them on a context that had run an SST call before."""
    c = kvsep.Context(0)
    try:
        d = torch.zeros(16, dtype=torch.uint8, device=DEV)
        z = torch.zeros(1, dtype=torch.int64, device=DEV)  # off / len: never read
        out = torch.zeros(1, dtype=torch.int32, device=DEV)
        for form in ("verify", "list", "salvage"):
            w = torch.full((4,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)  # first_bad, nbad, end, nkept
            if form == "verify":
                c.sst_verify_device(d.data_ptr(), z, z, out, w[0:1], w[1:2], count=0, total_bytes=0)
            elif form == "list":
                c.sst_verify_list_device(d.data_ptr(), z, z, out, w[0:1], w[1:2], bad_idx=z, bad_cap=1, count=0,
                                         total_bytes=0)
            else:
                ok = torch.zeros(1, dtype=torch.uint8, device=DEV)
                c.sst_salvage_device(d.data_ptr(), z, z, out, ok, d, 16, z, w[2:3], first_bad=w[0:1], nbad=w[1:2],
                                     nkept=w[3:4], count=0, total_bytes=0)
            torch.cuda.synchronize()
            assert w[:2].tolist() == [-1, 0], form
            if form == "salvage":
                assert w[2:].tolist() == [0, 0]
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ log / MANIFEST
def test_log_verify_device_matches_the_host_path(ctx, oracle):
    """A log image with records corrupted in two different 32 KiB blocks: ok[] from the device form equals
    kvsep_log_verify_host's, and kvsep_log_accept on it gives the host path's result."""
    rng = np.random.default_rng(77)
    records = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 6000, 40)]
    image, phys = FB.log_image(records, oracle)
    assert len(image) > 3 * FB.BLOCK
    img = bytearray(image)
    hit = []
    for blk in (0, 2):  # a payload byte of the second record of each block
        recs = [p for p in phys if p[0] // FB.BLOCK == blk and p[2] > 0]
        hdr = recs[1][0]
        img[hdr + FB.HEADER] ^= 0x04
        hit.append(hdr)
    img = bytes(img)
    off, ln, stored, _ = kvsep.log_walk(img)
    n = off.size
    host_ok = ctx.log_verify(img)
    assert int((host_ok == 0).sum()) == 2 and sorted(int(o) - 6 for o in off[host_ok == 0]) == sorted(hit)
    d = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
    g = Guarded(0, n)
    ctx.log_verify_device(d.data_ptr(), i64(off), i64(ln), i32(stored), g.ok, total_bytes=int(ln.sum()),
                          max_len=int(ln.max()))
    torch.cuda.synchronize()
    g.check(np.flatnonzero(host_ok == 0), True, "log")
    dev_ok = g.ok_all.cpu().numpy()[8 * GUARD:8 * GUARD + n]
    assert np.array_equal(dev_ok, host_ok)
    acc_d, drop_d = kvsep.log_accept(off, dev_ok, len(img))
    acc_h, drop_h = kvsep.log_accept(off, host_ok, len(img))
    assert np.array_equal(acc_d, acc_h) and drop_d == drop_h and drop_d > 0
    assert int((acc_d == 0).sum()) > 2  # the records after each bad one, to the end of its block, go with it


# ------------------------------------------------------------------------------------------------ group
def test_group_list_merges_the_shards(pool, oracle):
    """Two shards on members [0, 0], each with an index_base of its own and bad blocks in both: the merged list is the
    ascending global one, cut by a cap that falls inside the second shard."""
    shards_b = [Batch(pool, oracle, 700, 31), Batch(pool, oracle, TILE + 300, 32)]
    index_base = [5000, 100000]
    stored = [b.stored("half", seed=40 + k) for k, b in enumerate(shards_b)]
    truth = [np.flatnonzero(mask(b.crc) != s) + ib for b, s, ib in zip(shards_b, stored, index_base)]
    merged = np.concatenate(truth)
    assert truth[0].size > 10 and truth[1].size > 10 and np.all(np.diff(merged) > 0)
    outs = [torch.zeros(b.n, dtype=torch.int32, device=DEV) for b in shards_b]
    shards = [dict(base=b.data.data_ptr(), off=b.d_off, len=b.d_len, out=o, total_bytes=b.total, max_len=b.max_len)
              for b, o in zip(shards_b, outs)]
    ex = [i32(s) for s in stored]
    torch.cuda.synchronize()  # the members' streams do not wait for the default stream
    g = kvsep.Group([0, 0])
    try:
        for cap in (truth[0].size + 3, merged.size, merged.size + 5, 1, 0):
            fb, nb, bad = g.verify_list_device(shards, ex, index_base, cap)
            assert (fb, nb) == (int(merged[0]), merged.size), cap
            assert bad.tolist() == merged[:cap].tolist(), cap
            assert (fb, nb) == g.batch_device(shards, expected_masked=ex, index_base=index_base)
        for b, o in zip(shards_b, outs):
            assert np.array_equal(u32(o), b.crc)
        # the shards' index ranges the other way round: still one ascending list
        fb, nb, bad = g.verify_list_device(shards, ex, [100000, 5000], merged.size)
        want = np.sort(np.concatenate([truth[0] - 5000 + 100000, truth[1] - 100000 + 5000]))
        assert bad.tolist() == want.tolist() and fb == int(want[0])
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ capture
def test_captured_list_calls_replay_on_the_current_payload(oracle):
    """reserve, then ONE graph holding two verify_list_device calls on one stream.  Each replay's lists match the
    payload it ran on: clean, then with a block damaged, then with another one instead.  Nothing is allocated under
    capture: one set is held, and a list call with more blocks than reserved fails at capture with KVSEP_EINVAL."""
    host = splitmix64_bytes(POOL, 0xCA97, 0)
    data = torch.from_numpy(host.copy()).to(DEV)
    pool = (host, data)
    a, b = Batch(pool, oracle, 2 * TILE + 9, 61), Batch(pool, oracle, TILE - 3, 62)
    big = Batch(pool, oracle, 4 * TILE + 1, 63)
    c = kvsep.Context(0)
    try:
        c.reserve(a.n, a.total)
        sa, sb = mask(a.crc), mask(b.crc)
        sa[[3, 2 * TILE]] ^= np.uint32(1)  # two stored words wrong from the start
        d_sa, d_sb = i32(sa), i32(sb)
        ga, gb = Guarded(a.n, a.n), Guarded(5, b.n)
        outs = [torch.zeros(x.n, dtype=torch.int32, device=DEV) for x in (a, b)]
        res = torch.zeros(4, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            c.verify_list_device(data.data_ptr(), a.d_off, a.d_len, d_sa, outs[0], res[0:1], res[1:2],
                                 bad_idx=ga.bad_idx, bad_cap=a.n, ok=ga.ok, total_bytes=a.total, max_len=a.max_len,
                                 stream=s)
            c.verify_list_device(data.data_ptr(), b.d_off, b.d_len, d_sb, outs[1], res[2:3], res[3:4],
                                 bad_idx=gb.bad_idx, bad_cap=5, total_bytes=b.total, max_len=b.max_len, stream=s)
        assert c.capture_sets() == (4, 1)
        big_stored, big_out = i32(mask(big.crc)), torch.zeros(big.n, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                c.verify_list_device(data.data_ptr(), big.d_off, big.d_len, big_stored, big_out, res[0:1], res[1:2],
                                     bad_idx=ga.bad_idx, bad_cap=8, total_bytes=big.total, max_len=big.max_len,
                                     stream=torch.cuda.current_stream())
        del g2

        def truth(x, stored, at):
            """Ground truth for the payload with byte `at` flipped (None: as generated)."""
            h = host.copy()
            if at is not None:
                h[at] ^= 0xFF
            return np.flatnonzero(mask(oracle.batch(h, x.off, x.ln, threads=16)) != stored)

        long_a = int(np.flatnonzero(a.ln > 0)[10])
        long_b = int(np.flatnonzero(b.ln > 0)[-1])
        for at in (None, int(a.off[long_a]), int(b.off[long_b])):
            if at is not None:
                data[at] ^= 0xFF
            ga.idx_all[GUARD:GUARD + ga.bad_cap] = FILL
            gb.idx_all[GUARD:GUARD + gb.bad_cap] = FILL
            ga.ok_all[8 * GUARD:8 * GUARD + a.n] = OK_FILL
            res.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            ta, tb = truth(a, sa, at), truth(b, sb, at)
            if at is not None:
                assert ta.size > 2 or tb.size > 0
            r = res.cpu().numpy().view(np.uint64)
            assert (int(r[0]), int(r[1])) == (int(ta[0]), ta.size), at
            assert (int(r[2]), int(r[3])) == (int(tb[0]) if tb.size else NONE, tb.size), at
            ga.check(ta, True, ("captured a", at))
            gb.check(tb, False, ("captured b", at))
            if at is not None:
                data[at] ^= 0xFF
        del g
        torch.cuda.synchronize()
        c.release_captures()
    finally:
        c.close()
