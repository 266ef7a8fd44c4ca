"""GPU: the salvage forms built on the offsets pass.

  * kvsep_sst_salvage_device on the reference-written tests/golden/ref_table.sst and on a synthetic 2,049-block table,
    with 0, 1 and every block damaged: the destination holds the passed blocks with their trailers, concatenated by
    numpy, and is untouched past *end;
  * kvsep_crc32c_salvage_device with keep_before = the first_bad of a verify call on mutants of
    tests/golden/ref_small.vlog with a bad record in the middle: exactly the records the corpus says the reference's
    VlogReader returned;
  * kvsep_vlog_frame_auto_device byte-identical to kvsep_vlog_frame_device fed the host's offsets.
"""
import json
import os

import numpy as np
import pytest

import framing_corpus as FC
import kvsep
from framing_builders import fnv64
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SKIP = kvsep.OFFSET_SKIP
CANARY, MARGIN = 0xA5, 256


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(oracle):
    """name -> (image, off, len): the reference TableBuilder's file, and 2,049 blocks of 0..300 bytes framed the same
    way ([block][type][Mask(Value(block || type)) LE32]) with the oracle's CRCs."""
    with open(os.path.join(HERE, "ref_framing.json")) as f:
        blocks = json.load(f)["sst"]["blocks"]
    with open(os.path.join(HERE, "ref_table.sst"), "rb") as f:
        ref = np.frombuffer(f.read(), np.uint8).copy()
    rng = np.random.default_rng(31)
    n = 2049
    ln = rng.integers(0, 301, n).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(ln + np.uint64(5))[:-1]]).astype(np.uint64)
    img = splitmix64_bytes(int(off[-1] + ln[-1]) + 5, 3, 0)
    for o, k in zip(off, ln):
        img[int(o + k)] = rng.integers(0, 2)
    crc = oracle.batch(img, off, ln + np.uint64(1), None, threads=4)
    for o, k, c in zip(off, ln, crc):
        img[int(o + k) + 1:int(o + k) + 5] = np.array([kvsep.mask(int(c))], "<u4").view(np.uint8)
    return {"reference": (ref, np.array([b[0] for b in blocks], np.uint64), np.array([b[1] for b in blocks], np.uint64)),
            "synthetic": (img, off, ln)}


@pytest.mark.parametrize("damage", ["none", "one", "every"])
@pytest.mark.parametrize("table", ["reference", "synthetic"])
def test_sst_salvage_keeps_exactly_the_blocks_that_pass(ctx, tables, table, damage):
    img, off, ln = tables[table]
    n = off.size
    bad = {"none": [], "one": [n // 2], "every": list(range(n))}[damage]
    hurt = img.copy()
    for k, i in enumerate(bad):  # a payload byte, the type byte or a byte of the stored word, in turn
        at = int(off[i]) + (int(ln[i]) // 2 if k % 3 == 0 and ln[i] else int(ln[i]) + k % 3)
        hurt[at] ^= 0x10
    kept = np.ones(n, bool)
    kept[bad] = False
    ext = np.where(kept, ln + np.uint64(5), 0).astype(np.uint64)
    want_off = np.where(kept, np.cumsum(ext, dtype=np.uint64) - ext, np.uint64(SKIP))
    parts = [img[int(o):int(o + k) + 5] for o, k, keep in zip(off, ln, kept) if keep]
    want = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    size = int((ln + np.uint64(5)).sum()) + MARGIN
    dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    res = torch.full((4,), -5, dtype=torch.int64, device=DEV)  # first_bad, nbad, end, nkept
    d_img = dev8(hurt)
    ctx.sst_salvage_device(d_img.data_ptr(), u64(off), u64(ln), out, ok, dst.data_ptr(), size, dst_off, res[2:3],
                           first_bad=res[0:1], nbad=res[1:2], nkept=res[3:4], max_len=int(ln.max()))
    torch.cuda.synchronize()
    first_bad, nbad, end, nkept = res.cpu().numpy().view(np.uint64).tolist()
    assert (first_bad, nbad) == (bad[0] if bad else SKIP, len(bad))
    assert np.array_equal(ok.cpu().numpy(), kept.astype(np.uint8))
    assert (end, nkept) == (want.size, n - len(bad))
    assert np.array_equal(dst_off.cpu().numpy().view(np.uint64), want_off)
    got = dst.cpu().numpy()
    assert np.array_equal(got[:end], want), "the passed blocks with their trailers, back to back"
    assert (got[end:] == CANARY).all(), "the destination past *end was written"
    if damage == "none":  # a handle (dst_off[i], len[i]) reads every block back: the salvaged image verifies
        fb = torch.zeros(2, dtype=torch.int64, device=DEV)
        ctx.sst_verify_device(dst.data_ptr(), dst_off, u64(ln), out, fb[0:1], fb[1:2], max_len=int(ln.max()))
        torch.cuda.synchronize()
        assert fb.tolist() == [-1, 0]


def test_sst_salvage_into_a_destination_that_is_too_small(ctx, tables):
    """A passed block that does not lie inside [0, dst_bytes) is not written; *end still says what was needed."""
    img, off, ln = tables["synthetic"]
    n, need = off.size, int((ln + np.uint64(5)).sum())
    room = need // 2
    dst = torch.full((need,), CANARY, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    ok = torch.zeros(n, dtype=torch.uint8, device=DEV)
    dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    end = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_img = dev8(img)
    ctx.sst_salvage_device(d_img.data_ptr(), u64(off), u64(ln), out, ok, dst.data_ptr(), room, dst_off, end,
                           max_len=int(ln.max()))
    torch.cuda.synchronize()
    assert end.item() == need
    ends = np.cumsum(ln + np.uint64(5))
    fits = int(ends[ends <= room][-1])
    got = dst.cpu().numpy()
    assert np.array_equal(got[:fits], img[:fits]) and (got[fits:] == CANARY).all()


def mid_record_mutants():
    doc, _ = FC.load("vlog")
    total = len(doc["intact"]["records"])
    ms = [(cls, m) for cls in ("vlog_payload", "vlog_crc") for m in doc["classes"][cls]
          if 0 < len(m["records"]) < total - 1 and m["drops"] and m["cut"] is None and not m["append"]]
    assert len(ms) >= 6
    return ms[::max(1, len(ms) // 12)]


def test_vlog_truncation_copy_returns_what_the_reference_reader_returned(ctx):
    """verify_device leaves first_bad on the device; salvage_device with keep_before = that word copies the records
    before it, header and payload -- the records the corpus recorded from the reference's VlogReader."""
    doc, base = FC.load("vlog")
    for cls, m in mid_record_mutants():
        what = FC.describe(cls, m)
        img = FC.mutate(base, m)
        want = FC.want_records(m, doc["intact"])
        off, ln, stored, _ = kvsep.vlog_walk(img)
        n = off.size
        d_img = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
        out = torch.zeros(n, dtype=torch.int32, device=DEV)
        res = torch.full((4,), -5, dtype=torch.int64, device=DEV)  # first_bad, nbad, end, nkept
        dst = torch.full((len(img) + MARGIN,), CANARY, dtype=torch.uint8, device=DEV)
        dst_off = torch.zeros(n, dtype=torch.int64, device=DEV)
        ctx.verify_device(d_img.data_ptr(), u64(off), u64(ln), torch.from_numpy(stored.view(np.int32)).to(DEV), out,
                          res[0:1], res[1:2], total_bytes=int(ln.sum()))
        ctx.salvage_device(d_img.data_ptr(), u64(off - np.uint64(8)), u64(ln + np.uint64(8)), dst.data_ptr(),
                           dst.numel(), dst_off, res[2:3], keep_before=res[0:1], nkept=res[3:4])
        torch.cuda.synchronize()
        first_bad, _, end, nkept = res.cpu().numpy().view(np.uint64).tolist()
        assert first_bad == nkept == len(want), what
        got = dst.cpu().numpy()
        at = dst_off.cpu().numpy().view(np.uint64)
        recs = [[int(ln[i]) + 8, fnv64(got[int(at[i]):int(at[i] + ln[i]) + 8].tobytes())] for i in range(nkept)]
        assert FC.first_difference(recs, want) is None, f"{what}: {FC.first_difference(recs, want)}"
        assert end == sum(r[0] for r in want) and np.array_equal(got[:end], np.frombuffer(img, np.uint8)[:end]), what
        assert (at[nkept:] == np.uint64(SKIP)).all() and (got[end:] == CANARY).all(), what


def test_vlog_frame_auto_is_vlog_frame_with_the_offsets_made_on_the_device(ctx):
    with open(os.path.join(HERE, "ref_small.vlog"), "rb") as f:
        img = f.read()
    off, ln, _, used = kvsep.vlog_walk(img)
    assert used == len(img)
    rng = np.random.default_rng(4)
    cuts = [sorted(rng.integers(0, int(k) + 1, 2).tolist()) for k in ln]  # each payload as three segments
    seg_off = np.array([[o, o + a, o + b] for o, (a, b) in zip(off.tolist(), cuts)], np.uint64).ravel()
    seg_len = np.array([[a, b - a, int(k) - b] for k, (a, b) in zip(ln, cuts)], np.uint64).ravel()
    first = np.arange(0, seg_len.size + 1, 3, dtype=np.uint64)
    count, nseg, total = ln.size, seg_len.size, int(ln.sum())
    rec_off, end = kvsep.vlog_frame_offsets(ln, MARGIN)
    size = end + MARGIN
    d_img = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
    d_so, d_sl, d_first = u64(seg_off), u64(seg_len), u64(first)
    images = []
    for auto in (False, True):
        seg_crc = torch.zeros(nseg, dtype=torch.int32, device=DEV)
        crc_out = torch.zeros(count, dtype=torch.int32, device=DEV)
        dst = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
        if auto:
            d_rec = torch.full((count + 2,), -7, dtype=torch.int64, device=DEV)
            d_end = torch.full((3,), -7, dtype=torch.int64, device=DEV)
            ctx.vlog_frame_auto_device(d_img.data_ptr(), d_so, d_sl, d_first, seg_crc, crc_out, dst.data_ptr(), size,
                                       d_rec[1:count + 1], d_end[1:2], start=MARGIN, total_bytes=total)
            torch.cuda.synchronize()
            assert d_rec.cpu().numpy().view(np.uint64)[1:count + 1].tolist() == rec_off.tolist()
            assert d_rec[[0, -1]].tolist() == [-7, -7] and d_end.tolist() == [-7, end, -7]
        else:
            ctx.vlog_frame_device(d_img.data_ptr(), d_so, d_sl, d_first, seg_crc, crc_out, dst.data_ptr(), size,
                                  u64(rec_off), total_bytes=total)
            torch.cuda.synchronize()
        images.append((dst.cpu().numpy(), seg_crc.cpu().numpy(), crc_out.cpu().numpy()))
    for a, b in zip(*images):
        assert np.array_equal(a, b)
    assert np.array_equal(images[1][0][MARGIN:end], np.frombuffer(img, np.uint8))  # ... and both are the reference's file
