"""The scratch bracket every device form goes through (csrc/crc32c_device.hip with_scratch), one table of forms:

  growth    on a fresh context with no reserve, a one-element call on one stream, a 1,025-element call on a second
            stream (one past the 1,024 tile of the list, offsets and chain passes; a 2-block image for the log forms),
            the one-element call on the first stream again, none waited for in between: every array is reallocated
            behind its previous user (quiesce) and each call waits for the one before it on the other stream;
  capture   after reserve(1, 64) the 1,025-element call captured: KVSEP_EINVAL, no node in the graph, the capture set
            stays held; after release_captures and reserve(1025, ...) the same capture succeeds and its replay is exact;
  failure   the two forms that reach the CRC launch after other kernels (log_records, sst_table_verify) fail there by
            injection (a host-side error return) and the same call on another stream is exact: a failed body releases.

Every output is compared with the host form's.  Blocks and records are 64 bytes or less.
"""
import ctypes
import struct

import numpy as np
import pytest

import kvsep
import sst_tables as T
from framing_builders import log_image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import test_gpu_log_read as LR  # noqa: E402  (the reader's guarded arrays and host expectations)
import test_gpu_log_records as RC  # noqa: E402  (the chains' and records' guarded arrays and host expectations)
import test_gpu_sst_table as ST  # noqa: E402  (the SST forms' guarded outputs)

DEV = torch.device("cuda:0")
U64 = 0xFFFFFFFFFFFFFFFF
SKIP = U64
BIG = 1025


def dev(a, dtype):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).to(DEV).to(dtype)


def word(t, i=0):
    return int(t[i].item()) & U64


class Blocks:
    """n blocks of 1..64 bytes back to back, their CRCs from the host function, three of them reported wrong."""

    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        self.ln = rng.integers(1, 65, n).astype(np.uint64)
        self.off = np.concatenate([[0], np.cumsum(self.ln)[:-1]]).astype(np.uint64)
        self.data = kvsep.splitmix64_bytes(int(self.ln.sum()) + 64, seed, 0)
        raw = self.data.tobytes()
        self.crc = np.array([kvsep.value(raw[int(o):int(o + l)]) for o, l in zip(self.off, self.ln)], np.uint32)
        self.bad = sorted({0, n // 2, n - 1})
        self.stored = np.array([kvsep.mask(int(c)) for c in self.crc], np.uint32)
        self.stored[self.bad] ^= 0x10
        self.d_data = torch.from_numpy(self.data).to(DEV)
        self.d_off, self.d_ln = dev(self.off, torch.int64), dev(self.ln, torch.int64)
        self.d_stored = dev(self.stored, torch.int32)
        self.want_ok = np.ones(n, np.uint8)
        self.want_ok[self.bad] = 0


class VerifyList(Blocks):
    def __init__(self, n, oracle, seed=1):
        super().__init__(n, seed)
        self.out = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.words = torch.full((2,), 7, dtype=torch.int64, device=DEV)
        self.bad_idx = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)

    def call(self, ctx, stream):
        ctx.verify_list_device(self.d_data, self.d_off, self.d_ln, self.d_stored, self.out, self.words[0:1],
                               self.words[1:2], bad_idx=self.bad_idx, ok=self.ok, max_len=64, stream=stream)

    def check(self, what):
        assert np.array_equal(self.out.cpu().numpy().view(np.uint32), self.crc), what
        assert (word(self.words, 0), word(self.words, 1)) == (self.bad[0], len(self.bad)), what
        assert self.bad_idx.cpu().numpy()[:len(self.bad)].tolist() == self.bad, what
        assert np.array_equal(self.ok.cpu().numpy(), self.want_ok), what


class LogVerify(Blocks):
    def __init__(self, n, oracle, seed=2):
        super().__init__(n, seed)
        self.ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)

    def call(self, ctx, stream):
        ctx.log_verify_device(self.d_data, self.d_off, self.d_ln, self.d_stored, self.ok, max_len=64, stream=stream)

    def check(self, what):
        assert np.array_equal(self.ok.cpu().numpy(), self.want_ok), what


class Offsets:
    def __init__(self, n, oracle, seed=3):
        rng = np.random.default_rng(seed)
        self.ln = rng.integers(0, 65, n).astype(np.uint64)
        self.keep = (rng.random(n) < 0.8).astype(np.uint8)
        self.d_ln, self.d_keep = dev(self.ln, torch.int64), dev(self.keep, torch.uint8)
        self.dst_off = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.words = torch.full((2,), 7, dtype=torch.int64, device=DEV)

    def call(self, ctx, stream):
        ctx.offsets_device(self.d_ln, self.dst_off, self.words[0:1], keep=self.d_keep, head=2, tail=1, start=10,
                           nkept=self.words[1:2], stream=stream)

    def check(self, what):
        ext = np.where(self.keep != 0, self.ln + np.uint64(3), np.uint64(0))
        at = np.uint64(10) + np.concatenate([[0], np.cumsum(ext)[:-1]]).astype(np.uint64)
        want = np.where(self.keep != 0, at, np.uint64(SKIP))
        assert np.array_equal(self.dst_off.cpu().numpy().view(np.uint64), want), what
        assert (word(self.words, 0), word(self.words, 1)) == (10 + int(ext.sum()), int(self.keep.sum())), what


class Table:
    """A table of n data blocks of 8..64 bytes at restart interval 16, three data blocks damaged."""

    def __init__(self, n, seed):
        self.n = n
        img, self.off, self.ln, self.meta, self.index = T.build_table(n, 16, block_len=lambda i: 8 + (i * 37) % 57,
                                                                      seed=seed)
        self.bad = sorted({0, n // 2, n - 1})
        for i in self.bad:
            img[int(self.off[i]) + 3] ^= 1
        self.img = img
        raw = img.tobytes()
        self.crc = np.array([kvsep.value(raw[int(o):int(o + l) + 1]) for o, l in zip(self.off, self.ln)], np.uint32)
        self.d_img = ST.upload(img)
        self.want_ok = np.ones(n, np.uint8)
        self.want_ok[self.bad] = 0


class SstVerifyList(Table):
    def __init__(self, n, oracle, seed=4):
        super().__init__(n, seed)
        self.d_off, self.d_ln = dev(self.off, torch.int64), dev(self.ln, torch.int64)
        self.out = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.words = torch.full((2,), 7, dtype=torch.int64, device=DEV)
        self.bad_idx = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)

    def call(self, ctx, stream):
        ctx.sst_verify_list_device(self.d_img, self.d_off, self.d_ln, self.out, self.words[0:1], self.words[1:2],
                                   bad_idx=self.bad_idx, ok=self.ok, max_len=64, stream=stream)

    def check(self, what):
        assert np.array_equal(self.out.cpu().numpy().view(np.uint32), self.crc), what
        assert (word(self.words, 0), word(self.words, 1)) == (self.bad[0], len(self.bad)), what
        assert self.bad_idx.cpu().numpy()[:len(self.bad)].tolist() == self.bad, what
        assert np.array_equal(self.ok.cpu().numpy(), self.want_ok), what


class SstSalvage(Table):
    def __init__(self, n, oracle, seed=5):
        super().__init__(n, seed)
        self.d_off, self.d_ln = dev(self.off, torch.int64), dev(self.ln, torch.int64)
        self.out = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        self.dst_bytes = int(self.ln.sum()) + 5 * n
        self.dst = torch.full((self.dst_bytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        self.dst_off = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.words = torch.full((2,), 7, dtype=torch.int64, device=DEV)

    def call(self, ctx, stream):
        ctx.sst_salvage_device(self.d_img, self.d_off, self.d_ln, self.out, self.ok, self.dst, self.dst_bytes,
                               self.dst_off, self.words[0:1], nkept=self.words[1:2], max_len=64, stream=stream)

    def check(self, what):
        raw = self.img.tobytes()
        kept = [i for i in range(self.n) if self.want_ok[i]]
        want = b"".join(raw[int(self.off[i]):int(self.off[i] + self.ln[i]) + 5] for i in kept)
        at, pos = np.full(self.n, SKIP, np.uint64), 0
        for i in kept:
            at[i] = pos
            pos += int(self.ln[i]) + 5
        assert np.array_equal(self.ok.cpu().numpy(), self.want_ok), what
        assert np.array_equal(self.dst_off.cpu().numpy().view(np.uint64), at), what
        assert (word(self.words, 0), word(self.words, 1)) == (len(want), len(kept)), what
        h = self.dst.cpu().numpy()
        assert h[:len(want)].tobytes() == want and (h[len(want):] == 0xA5).all(), what


class VlogFrameAuto(Blocks):
    def __init__(self, n, oracle, seed=6):
        super().__init__(n, seed)
        self.first = dev(np.arange(n + 1, dtype=np.uint64), torch.int64)
        self.seg_crc = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.crc_out = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.dst_bytes = int(self.ln.sum()) + 8 * n
        self.dst = torch.full((self.dst_bytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        self.rec_off = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.end = torch.full((1,), 7, dtype=torch.int64, device=DEV)

    def call(self, ctx, stream):
        ctx.vlog_frame_auto_device(self.d_data, self.d_off, self.d_ln, self.first, self.seg_crc, self.crc_out, self.dst,
                                   self.dst_bytes, self.rec_off, self.end, max_len=64, stream=stream)

    def check(self, what):
        raw = self.data.tobytes()
        recs = [struct.pack("<II", kvsep.mask(int(c)), int(l)) + raw[int(o):int(o + l)]
                for c, o, l in zip(self.crc, self.off, self.ln)]  # db/value_log_writer.cc:46-76
        want = b"".join(recs)
        at = np.concatenate([[0], np.cumsum([len(r) for r in recs])[:-1]]).astype(np.uint64)
        assert np.array_equal(self.crc_out.cpu().numpy().view(np.uint32), self.crc), what
        assert np.array_equal(self.rec_off.cpu().numpy().view(np.uint64), at) and word(self.end) == len(want), what
        h = self.dst.cpu().numpy()
        assert h[:len(want)].tobytes() == want and (h[len(want):] == 0xA5).all(), what


def log_records_of(n, seed):
    """n records of 40..56 bytes: one record is one block short, 1,025 of them fill a block and part of the next."""
    rng = np.random.default_rng(seed)
    return [kvsep.splitmix64_bytes(int(rng.integers(40, 57)), seed + i, 0).tobytes() for i in range(n)]


class LogImage:
    def __init__(self, n, oracle, seed):
        self.img = bytearray(log_image(log_records_of(n, seed), oracle)[0])
        assert len(self.img) <= LR.BLOCK if n == 1 else LR.BLOCK < len(self.img) <= 2 * LR.BLOCK
        at = kvsep.log_walk(bytes(self.img))[0]
        self.img[int(at[n // 2]) + 3] ^= 1  # one record fails its checksum
        self.img = bytes(self.img)
        self.full = LR.host_full(self.img)
        self.cap = self.full[0][0].size + 3
        self.d = LR.upload(self.img)


class LogRead(LogImage):
    def __init__(self, n, oracle, seed=7):
        super().__init__(n, oracle, seed)
        self.a = LR.Arrays(self.cap)

    def call(self, ctx, stream):
        a = self.a
        ctx.log_read_device(self.d.data_ptr(), len(self.img), a.p("off"), a.p("len"), a.p("stored"), a.p("type"),
                            a.p("ok"), a.p("accept"), a.words[0:1], gap=a.p("gap"), dropped=a.words[1:2],
                            bad_length=a.words[2:3], cap=self.cap, stream=stream)

    def check(self, what):
        a, cap = self.a, self.cap
        walk, count, ok, accept, gap, dropped, bad_len = LR.host_expect(self.img, cap, self.full)
        assert a.word(0) == walk[0].size and not ok.all(), what
        for name, w, dt in (("off", walk[0], np.uint64), ("len", walk[1], np.uint64), ("stored", walk[2], np.uint32),
                            ("type", walk[3], np.uint8), ("ok", ok, np.uint8), ("accept", accept, np.uint8),
                            ("gap", gap, np.uint8)):
            assert np.array_equal(a.get(name, dt), LR.padded(w, cap, dt)), f"{what}: {name}"
        assert (a.word(1), a.word(2)) == (dropped, bad_len), what


class LogRecords(LogImage):
    def __init__(self, n, oracle, seed=8):
        super().__init__(n, oracle, seed)
        self.want = RC.host_records(self.img, self.cap, self.full)
        self.ra = RC.RecordArrays(self.cap, self.want["end"] + 40)

    def call(self, ctx, stream):
        self.ra.call(ctx, self.d.data_ptr(), len(self.img), stream=stream)

    def check(self, what):
        self.ra.check(self.want, what)


class LogChains:
    def __init__(self, n, oracle, seed=9):
        self.ty, self.accept, self.gap = RC.distribution("mix", n, np.random.default_rng(seed))
        self.n, self.cap = n, n + 3
        self.o = RC.ChainOut(self.cap)
        self.o.words[0] = n
        self.d = [RC.dev_in(a, self.cap, torch.uint8, 0xEE) for a in (self.ty, self.accept, self.gap)]

    def call(self, ctx, stream):
        o = self.o
        ctx.log_chains_device(self.d[0], self.d[1], o.words[0:1], o.first.p, o.whole.p, o.words[1:2], gap=self.d[2],
                              nwhole=o.words[2:3], cap=self.cap, stream=stream)

    def check(self, what):
        first, whole, nchain, nwhole, _ = RC.host_chains(self.ty, self.accept, self.gap, self.cap)
        o = self.o
        assert (o.word(0), o.word(1), o.word(2)) == (self.n, nchain, nwhole), what
        assert np.array_equal(o.first.get("first"), first) and np.array_equal(o.whole.get("whole"), whole), what


class LogFrame:
    """n records of 40..56 bytes appended to a log of 32,700 bytes: the first one already crosses a block end."""
    DEST = 32700

    def __init__(self, n, oracle, seed=10):
        recs = log_records_of(n, seed)
        self.n = n
        self.ln = np.array([len(r) for r in recs], np.uint64)
        self.off = np.concatenate([[0], np.cumsum(self.ln)[:-1]]).astype(np.uint64)
        self.src = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(DEV)
        self.d_off, self.d_ln = dev(self.off, torch.int64), dev(self.ln, torch.int64)
        # the host form: the image log::Writer appends, cut from the one it writes from offset 0 behind DEST zero bytes
        pad = [b"\0" * (self.DEST - 7)] if self.DEST else []
        self.want = log_image(pad + recs, oracle)[0][self.DEST:]
        self.rec_at, self.frag_first, self.nfrag, _ = kvsep.log_frame_layout(self.ln, dest_length=self.DEST)[:4]
        self.cap = int(self.nfrag) + 3
        self.dst = torch.full((len(self.want) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        self.o_rec_at = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        self.o_first = torch.full((n + 1,), -5, dtype=torch.int64, device=DEV)
        self.frag = [torch.full((self.cap,), -5, dtype=torch.int64, device=DEV) for _ in range(3)]
        self.frag_type = torch.full((self.cap,), 9, dtype=torch.uint8, device=DEV)
        self.frag_crc = torch.full((self.cap,), -5, dtype=torch.int32, device=DEV)
        self.words = torch.full((2,), 7, dtype=torch.int64, device=DEV)

    def call(self, ctx, stream):
        ctx.log_frame_device(self.src, self.d_off, self.d_ln, self.DEST, self.dst, len(self.want), self.o_rec_at,
                             self.o_first, self.frag[0], self.frag[1], self.frag[2], self.frag_type, self.frag_crc,
                             self.words[0:1], self.words[1:2], frag_cap=self.cap, total_bytes=int(self.ln.sum()),
                             stream=stream)

    def check(self, what):
        assert (word(self.words, 0), word(self.words, 1)) == (int(self.nfrag), len(self.want)), what
        assert np.array_equal(self.o_rec_at.cpu().numpy().view(np.uint64), np.asarray(self.rec_at, np.uint64)), what
        assert np.array_equal(self.o_first.cpu().numpy().view(np.uint64), np.asarray(self.frag_first, np.uint64)), what
        h = self.dst.cpu().numpy()
        assert h[:len(self.want)].tobytes() == bytes(self.want) and (h[len(self.want):] == 0xA5).all(), what


class SstIndex(Table):
    def __init__(self, n, oracle, seed=11):
        super().__init__(n, seed)
        self.cap = n + 3
        self.handle = torch.tensor(list(self.index), dtype=torch.int64, device=DEV)
        self.o = ST.Outs(self.cap)

    def call(self, ctx, stream):
        o = self.o
        ctx.sst_index_device(self.d_img, self.img.size, self.handle, o.p("off"), o.p("len"), o.p("nblocks"),
                             o.p("status"), cap=self.cap, stream=stream)

    def check(self, what):
        block = self.img.tobytes()[self.index[0]:self.index[0] + self.index[1]]
        want_off, want_len, want_n, want_status = kvsep.sst_index_walk(block, cap=self.cap)
        o = self.o
        assert (o.word("nblocks"), o.word("status")) == (want_n, want_status) == (self.n, kvsep.SST_OK), what
        assert np.array_equal(o.get("off", np.uint64), want_off) and np.array_equal(o.get("len", np.uint64), want_len), what
        o.guards_intact()


class SstTableVerify(Table):
    def __init__(self, n, oracle, seed=12):
        super().__init__(n, seed)
        self.cap = n + 5
        self.o = ST.Outs(self.cap)

    def call(self, ctx, stream):
        ST.run_table(ctx, self.d_img, self.img.size, self.o, max_len_hint=64, stream=stream)

    def check(self, what):
        o, n = self.o, self.n
        assert (o.word("status"), o.word("nblocks"), o.word("nbad")) == (kvsep.SST_OK, n, len(self.bad)), what
        slots_off = np.concatenate([self.off, np.array([self.meta[0], self.index[0]], np.uint64)])
        slots_len = np.concatenate([self.ln, np.array([self.meta[1], self.index[1]], np.uint64)])
        assert np.array_equal(o.get("off", np.uint64), LR.padded(slots_off, self.cap, np.uint64)), what
        assert np.array_equal(o.get("len", np.uint64), LR.padded(slots_len, self.cap, np.uint64)), what
        assert np.array_equal(o.get("crc", np.uint32)[:n], self.crc), what
        assert np.flatnonzero(o.get("ok") == 0).tolist() == self.bad and o.word("first_bad") == self.bad[0], what
        assert o.get("bad_idx", np.uint64)[:len(self.bad)].tolist() == self.bad, what
        o.guards_intact()


FORMS = {"verify_list": VerifyList, "log_verify": LogVerify, "sst_verify_list": SstVerifyList, "offsets": Offsets,
         "sst_salvage": SstSalvage, "vlog_frame_auto": VlogFrameAuto, "log_read": LogRead, "log_chains": LogChains,
         "log_records": LogRecords, "log_frame": LogFrame, "sst_index": SstIndex, "sst_table_verify": SstTableVerify}


@pytest.fixture(scope="module")
def cases(oracle):
    """cases(form, n): the inputs, fresh output arrays and host expectations of one call of `form` over n elements."""
    return lambda form, n: FORMS[form](n, oracle)


@pytest.mark.parametrize("form", list(FORMS))
def test_growth_across_streams(form, cases):
    ctx = kvsep.Context(0)
    try:
        small, big, again = cases(form, 1), cases(form, BIG), cases(form, 1)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()  # the inputs were uploaded on the current stream
        small.call(ctx, s1)
        big.call(ctx, s2)
        again.call(ctx, s1)
        torch.cuda.synchronize()
        small.check(f"{form}: one element, first stream")
        big.check(f"{form}: {BIG} elements, second stream")
        again.check(f"{form}: one element, first stream again")
    finally:
        ctx.close()


hip = ctypes.CDLL("libamdhip64.so")
RELAXED = 2  # hipStreamCaptureModeRelaxed


def captured(stream, fn):
    """fn() captured on `stream` with the runtime's own calls -> (the graph, its node count, what fn raised)."""
    assert hip.hipStreamBeginCapture(ctypes.c_void_p(stream.cuda_stream), RELAXED) == 0
    raised = None
    try:
        fn()
    except kvsep.KvsepError as e:
        raised = e
    graph, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert hip.hipStreamEndCapture(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    return graph, n.value, raised


@pytest.mark.parametrize("form", list(FORMS))
def test_captured_without_reservation(form, cases):
    ctx = kvsep.Context(0)
    try:
        ctx.reserve(1, 64)  # capture sets exist, sized for one element
        big = cases(form, BIG)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph, nodes, raised = captured(s, lambda: big.call(ctx, s))
        hip.hipGraphDestroy(graph)
        assert raised is not None and "(-1)" in str(raised), f"{form}: {raised}"  # KVSEP_EINVAL
        assert nodes == 0, f"{form}: a refused capture left {nodes} nodes in the graph"
        assert ctx.capture_sets()[1] == 1, f"{form}: the set the refused capture claimed stays held"
        ctx.release_captures()
        ctx.reserve(BIG + 8, 1 << 20)
        graph, nodes, raised = captured(s, lambda: big.call(ctx, s))
        assert raised is None and nodes > 0, f"{form}: {raised}"
        ex = ctypes.c_void_p()
        assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, ctypes.c_size_t(0)) == 0
        assert hip.hipGraphLaunch(ex, ctypes.c_void_p(s.cuda_stream)) == 0
        torch.cuda.synchronize()
        big.check(f"{form}: the replay of the reserved capture")
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(graph)
        ctx.release_captures()
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["log_records", "sst_table_verify"])
def test_failed_body_releases(form, cases, monkeypatch):
    monkeypatch.setenv("KVSEP_TEST_HOOKS", "1")
    ctx = kvsep.Context(0)
    try:
        failed, after = cases(form, BIG), cases(form, BIG)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.inject_failure()
        with pytest.raises(kvsep.KvsepError, match=r"\(-2\).*injected"):  # KVSEP_EHIP
            failed.call(ctx, s1)
        after.call(ctx, s2)
        torch.cuda.synchronize()
        after.check(f"{form}: the call after a failed one, on another stream")
    finally:
        ctx.close()
