"""The log / MANIFEST write side on the device: kvsep_log_frame_device against kvsep_log_frame_host, log::Writer's loop
restated here, the oracle's checksums and the committed reference file -- never against the device path itself.

  reference    the 12 records of tests/golden/ref_manifest.log, uploaded back to back, reproduce the file byte for byte,
               in one call and in two calls split after record 5 with dest_length carried over.
  edges        the start offsets and lengths of the CPU program's list, three records a call.
  rows         63 / 64 / 65 / 1,025 records of 4,673..4,680 bytes (resets inside rows and at their edges), lengths
               0..40, and a keep mask that drops every third record, whose off is KVSEP_OFFSET_SKIP.
  long         one 3 MiB record among small ones at frag_cap = nfrag, nfrag - 1 and nfrag + 3.
  destination  dst one byte short; a source at base + 3 and a dst at + 5.
  round trip   the image read back by kvsep_log_records_device; five mutants of the log corpus carried from bytes to a
               rewritten image on the device, which the host reader then reads as the reference's records.
  capture      reserve, then the reader and the writer in one graph, replayed over an image rewritten in place.
Every output array lies between guard elements and dst between guard bytes."""
import os
import struct

import numpy as np
import pytest

import kvsep
import framing_corpus as FC
from framing_builders import BLOCK, HEADER, FIRST, FULL, LAST, MIDDLE, fnv64, log_image, writer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import test_gpu_log_read as LR  # noqa: E402  (upload, the corpus reader's expectations)
import test_gpu_log_records as RC  # noqa: E402  (the guarded arrays of the records form)

DEV = torch.device("cuda:0")
G, S64, S8 = LR.G, LR.S64, LR.S8
U64 = 0xFFFFFFFFFFFFFFFF
SKIP = U64
DG = 64  # guard bytes on each side of dst
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Frame:
    """The outputs of one call between guards, and the source on the device."""

    def __init__(self, records, keep, frag_cap, dst_bytes, src_shift=0, dst_shift=0):
        n = len(records)
        self.count, self.frag_cap, self.dst_bytes, self.dst_shift = n, frag_cap, dst_bytes, dst_shift
        src, off = bytearray(b"\xEE" * (16 + src_shift)), []
        for r, k in zip(records, keep):
            off.append(len(src) - src_shift if k else SKIP)
            if k:
                src += r
        self.src_len = len(src)
        self.src = torch.frombuffer(bytearray(bytes(src) + b"\xEE" * 16), dtype=torch.uint8).to(DEV)
        self.base = self.src[src_shift:].data_ptr()
        self.off = torch.from_numpy(np.array(off, np.uint64).view(np.int64)).to(DEV) if n else None
        # a dropped record's length is read by nobody: junk
        ln = [len(r) if k else 0x7FFFFFFFFFFF for r, k in zip(records, keep)]
        self.len = torch.from_numpy(np.array(ln, np.uint64).view(np.int64)).to(DEV) if n else None
        self.keep = None if all(keep) else torch.from_numpy(np.array(keep, np.uint8)).to(DEV)
        self.total = sum(len(r) for r, k in zip(records, keep) if k)
        self.rec_at, self.frag_first = RC.Guarded(n, torch.int64), RC.Guarded(n + 1, torch.int64)
        self.frag_off, self.frag_len, self.frag_at = (RC.Guarded(frag_cap, torch.int64) for _ in range(3))
        self.frag_type, self.frag_crc = RC.Guarded(frag_cap, torch.uint8), RC.Guarded(frag_cap, torch.int32)
        self.words = torch.full((4,), S64, dtype=torch.int64, device=DEV)  # nfrag, written
        self.dst = torch.full((dst_bytes + 2 * DG + dst_shift,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(self, c, dest_length, stream=None, off=None, length=None, keep=None, base=None, count=None, total=None):
        c.log_frame_device(self.base if base is None else base, self.off if off is None else off,
                           self.len if length is None else length, dest_length, self.dst[DG + self.dst_shift:],
                           self.dst_bytes, self.rec_at.p, self.frag_first.p, self.frag_off.p, self.frag_len.p,
                           self.frag_at.p, self.frag_type.p, self.frag_crc.p, self.words[0:1], self.words[1:2],
                           keep=self.keep if keep is None else keep, count=self.count if count is None else count,
                           frag_cap=self.frag_cap, total_bytes=self.total if total is None else total, stream=stream)

    def word(self, i):
        return int(self.words[i].item()) & U64

    def body(self, what):
        h = self.dst.cpu().numpy()
        lo = DG + self.dst_shift
        assert (h[:lo] == 0xA5).all() and (h[lo + self.dst_bytes:] == 0xA5).all(), f"{what}: bytes around dst"
        return h[lo:lo + self.dst_bytes]


def expect(ctx, records, keep, dest_length, frag_cap, dst_bytes):
    """Everything a call writes, from kvsep_log_frame_host, kvsep_log_frame_layout and the loop above."""
    lens = [len(r) for r in records]
    host = ctx.log_frame([r for r, k in zip(records, keep) if k], dest_length=dest_length)
    phys, pads, end = writer(lens, keep, dest_length)
    assert end == len(host)
    rec_at, frag_first, nfrag, written = kvsep.log_frame_layout(lens, None if all(keep) else keep, dest_length)
    assert (nfrag, written) == (len(phys), len(host))
    want_at = np.full(len(records), SKIP, np.uint64)
    want_first = np.zeros(len(records) + 1, np.uint64)
    for f, p in reversed(list(enumerate(phys))):
        if p[4] == 0:
            want_at[p[3]] = p[0]
    k = 0
    for r in range(len(records) + 1):
        while k < len(phys) and phys[k][3] < r:
            k += 1
        want_first[r] = k
    assert np.array_equal(rec_at, want_at) and np.array_equal(frag_first, want_first), "kvsep_log_frame_layout"
    fo, fl, ft = np.zeros(frag_cap, np.uint64), np.zeros(frag_cap, np.uint64), np.zeros(frag_cap, np.uint8)
    fa, fc = np.full(frag_cap, SKIP, np.uint64), np.zeros(frag_cap, np.uint32)
    src_off, p = [], 16  # Frame lays the kept records back to back behind 16 guard bytes
    for r, kp in zip(records, keep):
        src_off.append(p)
        p += len(r) if kp else 0
    img = np.full(dst_bytes, 0xA5, np.uint8)
    hb = np.frombuffer(host, np.uint8)
    for f, (at, t, n, r, rpos) in enumerate(phys[:frag_cap]):
        fo[f], fl[f], fa[f], ft[f] = src_off[r] + rpos, n, at, t
        masked, hl, ht = struct.unpack_from("<IHB", host, at)
        assert (hl, ht) == (n, t), "the restated loop against kvsep_log_frame_host"
        fc[f] = kvsep.lib().kvsep_crc32c_unmask(masked)
        if at + HEADER + n <= dst_bytes:
            img[at:at + HEADER + n] = hb[at:at + HEADER + n]
    for at, n, r in pads:
        if want_first[r] < frag_cap and at + n <= dst_bytes:
            img[at:at + n] = 0
    return dict(rec_at=want_at, frag_first=want_first, frag_off=fo, frag_len=fl, frag_at=fa, frag_type=ft, frag_crc=fc,
                nfrag=len(phys), written=len(host), img=img, host=host)


def check(ctx, records, dest_length, what, keep=None, cap_delta=0, dst_delta=0, src_shift=0, dst_shift=0, stream=None):
    keep = [1] * len(records) if keep is None else keep
    lens = [len(r) for r in records]
    phys, _, end = writer(lens, keep, dest_length)
    frag_cap, dst_bytes = max(len(phys) + cap_delta, 0), max(end + dst_delta, 0)
    want = expect(ctx, records, keep, dest_length, frag_cap, dst_bytes)
    fr = Frame(records, keep, frag_cap, dst_bytes, src_shift, dst_shift)
    fr.call(ctx, dest_length, stream=stream)
    torch.cuda.synchronize()
    compare(fr, want, what)
    h = fr.src.cpu().numpy()
    assert (h[:16 + src_shift] == 0xEE).all() and (h[fr.src_len:] == 0xEE).all(), f"{what}: the source changed"
    return fr, want


def compare(fr, want, what):
    assert (fr.word(0), fr.word(1)) == (want["nfrag"], want["written"]), f"{what}: *nfrag / *written"
    assert fr.word(2) == S64 & U64 and fr.word(3) == S64 & U64
    for name in ("rec_at", "frag_first", "frag_off", "frag_len", "frag_at", "frag_type"):
        assert np.array_equal(getattr(fr, name).get(name), want[name]), f"{what}: {name}"
    assert np.array_equal(fr.frag_crc.get("frag_crc").view(np.uint32), want["frag_crc"]), f"{what}: frag_crc"
    body = fr.body(what)
    bad = np.flatnonzero(body != want["img"])
    assert bad.size == 0, f"{what}: dst differs from the host image at {int(bad[0])} of {body.size}"


def payload(n, seed=0):
    return kvsep.splitmix64_bytes(n + 1, 77 + seed, 0)[:n].tobytes()


# ------------------------------------------------------------------ the reference file
@pytest.fixture(scope="module")
def manifest_records():
    import json
    with open(os.path.join(GOLDEN, "ref_framing.json")) as f:
        lg = json.load(f)["log"]
    data = kvsep.splitmix64_bytes(int(sum(lg["lens"])) + 1, lg["seed"], 0)
    out, p = [], 0
    for n in lg["lens"]:
        out.append(data[p:p + n].tobytes())
        p += n
    with open(os.path.join(GOLDEN, "ref_manifest.log"), "rb") as f:
        return out, f.read()


def test_reference_manifest_byte_for_byte(ctx, manifest_records):
    recs, manifest = manifest_records
    assert len(recs) == 12 and len(manifest) == 327720
    fr, want = check(ctx, recs, 0, "the 12 reference records")
    assert want["nfrag"] == 19 and fr.body("reference").tobytes() == manifest
    a, _ = check(ctx, recs[:5], 0, "records 0..4")
    b, _ = check(ctx, recs[5:], a.word(1), "records 5..11 at dest_length")
    assert a.body("a").tobytes() + b.body("b").tobytes() == manifest


# ------------------------------------------------------------------ edges
def edge_lengths(start):
    b = 0 if start > 32761 else start
    avail = 32761 - b
    return [0, 1, 6, 7, 8, max(avail - 1, 0), avail, avail + 1, 32760, 32761, 32762, 65521, 65522, 65523, 100000]


@pytest.mark.parametrize("start", [0, 7, 32754, 32760, 32761, 32762, 32767])
def test_edges_three_records_a_call(ctx, start):
    L = edge_lengths(start)
    pool = {n: payload(n, n % 13) for n in set(L)}
    for a in range(len(L)):  # every length first, second and third, against different neighbours
        trio = [L[a], L[(a + 4) % len(L)], L[(a + 9) % len(L)]]
        check(ctx, [pool[n] for n in trio], start + BLOCK * (a % 3), f"start {start}, lengths {trio}")


# ------------------------------------------------------------------ rows
@pytest.mark.parametrize("count", [63, 64, 65, 1025])
def test_rows_with_resets_inside_and_at_their_edges(ctx, count):
    rng = np.random.default_rng(count)
    big = payload(4680 * 4, 3)
    recs = [big[int(o):int(o) + int(n)] for o, n in zip(rng.integers(0, 4680 * 3, count), rng.integers(4673, 4681, count))]
    check(ctx, recs, 0, f"{count} records of 4,673..4,680 bytes")
    check(ctx, recs, 32765, f"{count} records behind a pad")
    small = [big[:int(n)] for n in rng.integers(0, 41, count)]
    check(ctx, small, 32700, f"{count} records of 0..40 bytes")
    keep = [0 if i % 3 == 2 else 1 for i in range(count)]
    check(ctx, recs, 11, f"{count} records, every third dropped", keep=keep)
    check(ctx, recs, 11, f"{count} records, all dropped", keep=[0] * count)


def test_no_records(ctx):
    check(ctx, [], 32766, "no records", cap_delta=3)


# ------------------------------------------------------------------ a long record, frag_cap around nfrag
@pytest.mark.parametrize("cap_delta", [0, -1, 3])
def test_long_record_among_small_ones(ctx, cap_delta):
    recs = [payload(100, 1), payload(5000, 2), payload(3 << 20, 3), payload(0), payload(32761, 4), payload(9, 5)]
    fr, want = check(ctx, recs, 32000, f"a 3 MiB record, frag_cap = nfrag {cap_delta:+d}", cap_delta=cap_delta)
    assert want["nfrag"] > 97 and fr.word(0) == want["nfrag"]
    if cap_delta < 0:  # the written prefix is the host image up to the first fragment not stored
        cut = int(writer([len(r) for r in recs], [1] * len(recs), 32000)[0][want["nfrag"] - 1][0])
        body = fr.body("cut")
        assert body[:cut].tobytes() == want["host"][:cut] and (body[cut:] == 0xA5).all()


# ------------------------------------------------------------------ the destination
def test_dst_one_byte_short_and_unaligned_placement(ctx):
    recs = [payload(4674, i) for i in range(20)] + [payload(70000, 9)]
    fr, want = check(ctx, recs, 5, "dst one byte short", dst_delta=-1)
    last = writer([len(r) for r in recs], [1] * len(recs), 5)[0][-1][0]
    assert fr.word(1) == want["written"] == fr.dst_bytes + 1 and (fr.body("short")[last:] == 0xA5).all()
    check(ctx, recs, 32763, "a source at base + 3, a dst at + 5", src_shift=3, dst_shift=5)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    check(ctx, recs, 0, "a caller's own stream", stream=s)


# ------------------------------------------------------------------ round trips through the device reader
def read_back(ctx, img):
    """kvsep_log_records_device over a host image -> (the arrays, the records it assembled)."""
    cap = kvsep.log_walk(img)[0].size + 3
    d = LR.upload(img)
    ra = RC.RecordArrays(cap, len(img) + 40)
    ra.call(ctx, d.data_ptr(), len(img))
    torch.cuda.synchronize()
    o = ra.o
    off, ln, whole = o.rec_off.get("rec_off"), o.rec_len.get("rec_len"), o.whole.get("whole")
    h = ra.dst.cpu().numpy()[64:]
    return ra, [h[int(a):int(a) + int(n)].tobytes() for a, n, w in zip(off, ln, whole) if w]


def test_written_image_reads_back_as_the_records(ctx):
    recs = [payload(n, i) for i, n in enumerate([0, 1, 32761, 40000, 7, 4674, 4674, 4674, 4674, 4674, 4674, 4674, 131072, 3])]
    fr, want = check(ctx, recs, 0, "round trip")
    _, got = read_back(ctx, fr.body("round trip").tobytes())
    assert got == recs


MUTANT_CLASSES = ["log_crc", "log_length", "log_zero_header", "log_chain_gap", "log_truncate_pad"]


@pytest.mark.parametrize("cls", MUTANT_CLASSES)
def test_damaged_log_rewritten_on_the_device(ctx, cls):
    """bytes -> log_records_device -> log_frame_device with rec_off / rec_len / whole as they are -> an image whose host
    walk, verdicts, accept rule and kvsep_log_chains give exactly the records the reference reader returned."""
    doc, base = FC.load("log")
    m = doc["classes"][cls][len(doc["classes"][cls]) // 2]
    what = FC.describe(cls, m)
    img = FC.mutate(base, m)
    ra, recs = read_back(ctx, img)
    cap = ra.a.cap
    nfrag = 2 * cap + len(img) // 32761 + 1  # the documented bound
    fr = Frame([b""] * cap, [1] * cap, nfrag, len(img) + 7 * cap + 64)
    o = ra.o
    fr.call(ctx, 0, off=o.rec_off.p, length=o.rec_len.p, keep=o.whole.p, base=ra.dst[64:].data_ptr(), count=cap,
            total=len(img))
    torch.cuda.synchronize()
    written = fr.word(1)
    out = fr.body(what)[:written].tobytes()
    assert out == ctx.log_frame(recs, dest_length=0), what  # what the host writer makes of the same records
    off, ln, stored, ty = kvsep.log_walk(out)
    ok = FC.log_host_ok(out, off, ln, stored)
    accept, gap, dropped, _ = kvsep.log_accept_gaps(out, ok)
    first, whole, nchain, _ = kvsep.log_chains(ty, accept, gap)
    got = []
    for j in range(nchain):
        if whole[j]:
            r = b"".join(out[int(off[i]) + 1:int(off[i]) + int(ln[i])] for i in range(int(first[j]), int(first[j + 1])))
            got.append([len(r), fnv64(r)])
    assert dropped == 0 and ok.all()
    diff = FC.first_difference(got, FC.want_records(m, doc["intact"]))
    assert diff is None, f"{what}: {diff}"


# ------------------------------------------------------------------ capture
def test_captured_reader_and_writer_follow_each_replay():
    """reserve, then log_records_device and log_frame_device in one graph; the image is rewritten in place."""
    doc, base = FC.load("log")
    intact = base
    damaged = FC.mutate(base, doc["classes"]["log_crc"][len(doc["classes"]["log_crc"]) // 2])
    assert len(damaged) == len(intact)
    n = len(intact)
    cap = kvsep.log_walk(intact)[0].size + 3
    nfrag = 2 * cap + n // 32761 + 1
    c = kvsep.Context(0)
    try:
        d = LR.upload(intact)
        ra = RC.RecordArrays(cap, n + 40)
        fr = Frame([b""] * cap, [1] * cap, nfrag, n + 7 * cap + 64)
        c.reserve(max(cap, nfrag, n // BLOCK + 1), n)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            ra.call(c, d.data_ptr(), n, stream=s)
            fr.call(c, 0, stream=s, off=ra.o.rec_off.p, length=ra.o.rec_len.p, keep=ra.o.whole.p,
                    base=ra.dst[64:].data_ptr(), count=cap, total=n)
        assert c.capture_sets()[1] == 1
        lens = []
        for img in (intact, damaged, intact):
            d[:n] = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
            fr.dst.fill_(0xA5)
            g.replay()
            torch.cuda.synchronize()
            want = RC.host_records(img, cap)
            host = c.log_frame(want["recs"], dest_length=0)
            assert fr.word(1) == len(host) and fr.body("replay")[:len(host)].tobytes() == host
            assert (fr.body("replay")[len(host):] == 0xA5).all()
            lens.append(len(host))
        assert lens[1] < lens[0] == lens[2]
        # a call over the reservation: refused at capture, nothing enqueued, the sentinel words untouched
        over = max(cap, nfrag, n // BLOCK + 1) + 1
        big = Frame([b""] * 2, [1, 1], over, 64)
        torch.cuda.synchronize()
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                big.call(c, 0, stream=torch.cuda.current_stream())
        del g2
        torch.cuda.synchronize()
        assert (big.words.cpu().numpy() == S64).all() and big.rec_at.untouched() and big.frag_first.untouched()
        assert big.frag_at.untouched() and bool((big.dst == 0xA5).all().item())
        del g
        c.release_captures()
    finally:
        c.close()


def test_refusals_leave_everything_untouched(ctx):
    fr = Frame([b"ab", b"c"], [1, 1], 4, 64)
    for kw, msg in ((dict(off=0), "null base, off, len"), (dict(count=1 << 32), r"2\^32")):
        with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*" + msg):
            if "off" in kw:
                ctx.log_frame_device(fr.base, None, fr.len, 0, fr.dst, 64, fr.rec_at.p, fr.frag_first.p, fr.frag_off.p,
                                     fr.frag_len.p, fr.frag_at.p, fr.frag_type.p, fr.frag_crc.p, fr.words[0:1],
                                     fr.words[1:2], count=2, frag_cap=4)
            else:
                fr.call(ctx, 0, **kw)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null frag_first, nfrag or written"):
        ctx.log_frame_device(fr.base, fr.off, fr.len, 0, fr.dst, 64, fr.rec_at.p, fr.frag_first.p, fr.frag_off.p,
                             fr.frag_len.p, fr.frag_at.p, fr.frag_type.p, fr.frag_crc.p, None, fr.words[1:2], count=2,
                             frag_cap=4)
    torch.cuda.synchronize()
    assert (fr.words.cpu().numpy() == S64).all() and fr.rec_at.untouched() and fr.frag_at.untouched()
    assert bool((fr.dst == 0xA5).all().item())
