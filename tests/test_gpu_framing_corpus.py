"""The corpus of damaged framing files (tests/golden/framing_corpus_*.json: what the reference's log::Reader,
VlogReader and ReadBlock returned and reported on every mutant, tests/golden/make_framing_corpus.py) through the entry
points that run on the device.  One test per mutation class; the images are at most 330 KB.

  log    kvsep_log_verify_host (ctx.log_verify) and kvsep_log_verify_device on the uploaded image with the walk's
         arrays -- auto route, set_kernel("wide"), set_kernel("narrow") -- give the host leg's verdicts of
         test_framing_reference_cpu.py; kvsep_log_accept_gaps and the assembly loop on them give log::Reader's records
         and its "checksum mismatch" / "bad record length" bytes.
  vlog   kvsep_vlog_verify_host and a 2-member group [0, 0] through kvsep_vlog_verify_host_group: ngood, good_bytes
         and drop_bytes as VlogReader saw them.
  SST    kvsep_sst_verify_device / _host and the list forms: first_bad, nbad and the ascending bad_idx, with a bad_cap
         below, at and above nbad, name exactly the blocks ReadBlock rejected.
"""
import numpy as np
import pytest

import kvsep
import framing_corpus as FC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
SENTINEL = -7


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def group():
    g = kvsep.Group([0, 0])
    yield g
    g.close()


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def dev_bytes(img):
    return torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)


# ------------------------------------------------------------------ log / MANIFEST
@pytest.mark.parametrize("cls", FC.classes("log"))
def test_log_corpus(ctx, cls):
    doc, base = FC.load("log")
    try:
        for m in doc["classes"][cls]:
            what = FC.describe(cls, m)
            img = FC.mutate(base, m)
            walk = kvsep.log_walk(img)
            off, ln, stored, _ = walk
            n = off.size
            want_ok = FC.log_host_ok(img, off, ln, stored)
            host_ok = ctx.log_verify(img)
            assert np.array_equal(host_ok, want_ok), f"{what}: kvsep_log_verify_host"
            FC.check_log(cls, m, img, doc["intact"], walk, host_ok)
            if not n:
                continue
            d, d_off, d_ln, d_st = dev_bytes(img), dev_u64(off), dev_u64(ln), dev_u32(stored)
            for kernel in ("auto", "wide", "narrow"):
                ctx.set_kernel(kernel)
                ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
                ctx.log_verify_device(d.data_ptr(), d_off, d_ln, d_st, ok, total_bytes=int(ln.sum()),
                                      max_len=int(ln.max()))
                torch.cuda.synchronize()
                dev_ok = ok.cpu().numpy()
                assert np.array_equal(dev_ok, want_ok), f"{what}: kvsep_log_verify_device, kernel {kernel}"
            FC.check_log(cls, m, img, doc["intact"], walk, dev_ok)
    finally:
        ctx.set_kernel("auto")


# ------------------------------------------------------------------ vlog
@pytest.mark.parametrize("cls", FC.classes("vlog"))
def test_vlog_corpus(ctx, group, cls):
    doc, base = FC.load("vlog")
    for m in doc["classes"][cls]:
        what = FC.describe(cls, m)
        img = FC.mutate(base, m)
        ngood, good_bytes, drop, hit = FC.vlog_expect(m, doc["intact"])
        off, ln, _, _ = kvsep.vlog_walk(img)
        for form, got in (("kvsep_vlog_verify_host", ctx.vlog_verify(img, with_drop=True)),
                          ("kvsep_vlog_verify_host_group", group.vlog_verify(img))):
            assert got[0] == off.size, f"{what}: {form} nrecords"
            assert got[1:] == (ngood, good_bytes, drop), f"{what}: {form} gave {got[1:]}, reference " \
                                                          f"{(ngood, good_bytes, drop)}"
            assert (got[1] < got[0]) == hit, f"{what}: {form}: a checksum mismatch was reported"
        diff = FC.first_difference(FC.vlog_records(img, off, ln, ngood), FC.want_records(m, doc["intact"]))
        assert diff is None, f"{what}: {diff}"


# ------------------------------------------------------------------ SST
@pytest.mark.parametrize("cls", FC.classes("sst"))
def test_sst_corpus(ctx, cls):
    doc, base = FC.load("sst")
    blocks = doc["blocks"]
    off = np.array([b[0] for b in blocks], np.uint64)
    ln = np.array([b[1] for b in blocks], np.uint64)
    n, max_len = off.size, int(ln.max())
    d_off, d_ln = dev_u64(off), dev_u64(ln)
    for m in doc["classes"][cls]:
        what = FC.describe(cls, m)
        img = FC.mutate(base, m)
        bad = m["bad"]
        first = bad[0] if bad else -1
        d = dev_bytes(img)
        out = torch.zeros(n, dtype=torch.int32, device=DEV)
        fb = torch.zeros(1, dtype=torch.int64, device=DEV)
        nb = torch.zeros(1, dtype=torch.int64, device=DEV)
        ctx.sst_verify_device(d.data_ptr(), d_off, d_ln, out, fb, nb, max_len=max_len)
        torch.cuda.synchronize()
        assert (int(fb.item()), int(nb.item())) == (first, len(bad)), f"{what}: kvsep_sst_verify_device"
        crc = out.cpu().numpy().view(np.uint32)
        h_out, h_fb, h_nb = ctx.sst_verify(img, off, ln)
        assert (h_fb, h_nb) == (first, len(bad)), f"{what}: kvsep_sst_verify_host"
        assert np.array_equal(h_out, crc), what
        for cap in sorted({max(len(bad) - 1, 0), len(bad), len(bad) + 3}):
            kept = bad[:cap]
            idx = torch.full((cap + 4,), SENTINEL, dtype=torch.int64, device=DEV)
            ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
            fb.fill_(SENTINEL)
            nb.fill_(SENTINEL)
            ctx.sst_verify_list_device(d.data_ptr(), d_off, d_ln, out, fb, nb, bad_idx=idx, bad_cap=cap, ok=ok,
                                       max_len=max_len)
            torch.cuda.synchronize()
            assert (int(fb.item()), int(nb.item())) == (first, len(bad)), f"{what}: list device, cap {cap}"
            assert idx.cpu().tolist() == kept + [SENTINEL] * (cap + 4 - len(kept)), f"{what}: list device, cap {cap}"
            assert np.flatnonzero(ok.cpu().numpy() != 1).tolist() == bad and set(ok.cpu().tolist()) <= {0, 1}, what
            _, l_fb, l_nb, l_bad = ctx.sst_verify_list(img, off, ln, bad_cap=cap)
            assert (l_fb, l_nb, l_bad.tolist()) == (first, len(bad), kept), f"{what}: list host, cap {cap}"
