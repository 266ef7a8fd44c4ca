"""The device log / MANIFEST reader: kvsep_log_walk_device, kvsep_log_accept_gaps_device and kvsep_log_read_device
against the host walk (kvsep_log_walk), the library's host leg for the verdicts (framing_corpus.log_host_ok) and the
host accept rule (kvsep_log_accept_gaps) -- never against the device path itself.

  corpus       every mutant of the recorded log corpus at cap = count - 1, count and count + 3: the walk's arrays, the
               zero padding, untouched guard elements, ok / accept / gap and both byte counts; at cap >= count the
               assembled records and the reported bytes are log::Reader's own (tests/golden/framing_corpus_log.json).
  constructed  the smallest shapes at which the kernels can go wrong: sizes around 0, 7 and a block boundary, 4,681
               empty records in a block, a record of l = 32761, trailers of 1 to 6 bytes, 65 and 1,030 blocks, zero
               headers, bad lengths, dead parts of blocks, types 5 and 6, gaps across all-zero blocks, an image at
               base + 1 and base + 3 between guard bytes, a caller's own stream.
  accept       the accept pass alone on verdicts the test writes.
  capture      reserve, then the whole reader under torch.cuda.graph, replayed over an image rewritten in place."""
import struct

import numpy as np
import pytest

import kvsep
import framing_corpus as FC
from framing_builders import BLOCK, HEADER, assemble, log_image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
G = 4  # guard elements on each side of every output array
S64, S32, S8 = -7, -7, 7


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


class Arrays:
    """The reader's arrays for `cap` elements, each between G guard elements that must stay as they are."""

    def __init__(self, cap):
        self.cap = cap
        self.off = torch.full((cap + 2 * G,), S64, dtype=torch.int64, device=DEV)
        self.len = torch.full((cap + 2 * G,), S64, dtype=torch.int64, device=DEV)
        self.stored = torch.full((cap + 2 * G,), S32, dtype=torch.int32, device=DEV)
        self.type, self.ok, self.accept, self.gap = (torch.full((cap + 2 * G,), S8, dtype=torch.uint8, device=DEV)
                                                     for _ in range(4))
        self.words = torch.full((3,), S64, dtype=torch.int64, device=DEV)  # nrec, dropped, bad_length

    def p(self, name):
        return getattr(self, name)[G:]

    def get(self, name, dtype):
        a = getattr(self, name).cpu().numpy()
        sentinel = S8 if a.dtype == np.uint8 else S64
        assert (a[:G] == sentinel).all() and (a[G + self.cap:] == sentinel).all(), f"guard elements of {name}"
        return a[G:G + self.cap].view(dtype)

    def word(self, i):
        return int(self.words[i].item()) & 0xFFFFFFFFFFFFFFFF


def upload(img, shift=0):
    """The image at `shift` bytes into a tensor, 0xA5 guard bytes around it."""
    t = torch.full((len(img) + shift + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    if len(img):
        t[shift:shift + len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
    return t


def guards_intact(t, img, shift):
    h = t.cpu().numpy()
    return (h[:shift] == 0xA5).all() and (h[shift + len(img):] == 0xA5).all() and \
        h[shift:shift + len(img)].tobytes() == bytes(img)


def host_full(img):
    """(walk, verdicts) of the host walk and the library's host leg over every record: computed once per image."""
    walk = kvsep.log_walk(img)
    return walk, FC.log_host_ok(img, walk[0], walk[1], walk[2])


def host_expect(img, cap, full=None):
    """(walk, count, ok, accept, gap, dropped, bad_length) of the host functions for arrays of cap elements."""
    walk, ok = full if full is not None else host_full(img)
    count = min(walk[0].size, cap)
    ok = ok[:count]
    accept, gap, dropped, bad_len = kvsep.log_accept_gaps(img, ok)
    return walk, count, ok, accept, gap, dropped, bad_len


def padded(a, cap, dtype):
    out = np.zeros(cap, dtype)
    out[:min(a.size, cap)] = a[:cap]
    return out


def check_walk(ctx, d, n, cap, walk, what, stream=None):
    a = Arrays(cap)
    ctx.log_walk_device(d.data_ptr() if n else 0, n, a.words[0:1], off=a.p("off"), length=a.p("len"),
                        stored=a.p("stored"), type=a.p("type"), cap=cap, stream=stream)
    torch.cuda.synchronize()
    assert a.word(0) == walk[0].size, f"{what}: nrec, cap {cap}"
    for name, w, dt in (("off", walk[0], np.uint64), ("len", walk[1], np.uint64), ("stored", walk[2], np.uint32),
                        ("type", walk[3], np.uint8)):
        assert np.array_equal(a.get(name, dt), padded(w, cap, dt)), f"{what}: walk {name}, cap {cap}"
    assert a.word(1) == S64 & 0xFFFFFFFFFFFFFFFF  # the walk writes its own word only


def check_read(ctx, d, n, cap, expect, what, stream=None):
    walk, count, ok, accept, gap, dropped, bad_len = expect
    a = Arrays(cap)
    ctx.log_read_device(d.data_ptr(), n, a.p("off"), a.p("len"), a.p("stored"), a.p("type"), a.p("ok"),
                        a.p("accept"), a.words[0:1], gap=a.p("gap"), dropped=a.words[1:2], bad_length=a.words[2:3],
                        cap=cap, stream=stream)
    torch.cuda.synchronize()
    assert a.word(0) == walk[0].size, f"{what}: nrec, cap {cap}"
    for name, w, dt in (("off", walk[0], np.uint64), ("len", walk[1], np.uint64), ("stored", walk[2], np.uint32),
                        ("type", walk[3], np.uint8), ("ok", ok, np.uint8), ("accept", accept, np.uint8),
                        ("gap", gap, np.uint8)):
        assert np.array_equal(a.get(name, dt), padded(w, cap, dt)), f"{what}: read {name}, cap {cap}"
    assert (a.word(1), a.word(2)) == (dropped, bad_len), f"{what}: dropped / bad-length bytes, cap {cap}"
    return a


def check_image(ctx, img, what, shift=0, stream=None, caps=None):
    full = host_full(img)
    nrec = full[0][0].size
    d = upload(img, shift)
    base = d[shift:]
    for cap in caps if caps is not None else sorted({max(nrec - 1, 0), nrec, nrec + 3}):
        expect = host_expect(img, cap, full)
        check_walk(ctx, base, len(img), cap, expect[0], what, stream)
        check_read(ctx, base, len(img), cap, expect, what, stream)
    assert guards_intact(d, img, shift), f"{what}: the image or the bytes around it changed"


# ------------------------------------------------------------------ the recorded corpus
@pytest.mark.parametrize("cls", FC.classes("log"))
def test_log_corpus(ctx, cls):
    doc, base = FC.load("log")
    for m in doc["classes"][cls]:
        what = FC.describe(cls, m)
        img = FC.mutate(base, m)
        full = host_full(img)
        nrec = full[0][0].size
        d = upload(img)
        for cap in sorted({max(nrec - 1, 0), nrec, nrec + 3}):
            expect = host_expect(img, cap, full)
            walk = expect[0]
            check_walk(ctx, d, len(img), cap, walk, what)
            a = check_read(ctx, d, len(img), cap, expect, what)
            if cap < nrec:
                continue
            # the device outputs against what log::Reader returned and reported
            off, ln, ty = a.get("off", np.uint64)[:nrec], a.get("len", np.uint64)[:nrec], a.get("type", np.uint8)[:nrec]
            got = assemble(img, off, ln, ty, a.get("accept", np.uint8)[:nrec], a.get("gap", np.uint8)[:nrec])
            diff = FC.first_difference(got, FC.want_records(m, doc["intact"]))
            assert diff is None, f"{what}: {diff}"
            assert a.word(1) == FC.reported(m, FC.MISMATCH), f"{what}: checksum-mismatch bytes"
            assert a.word(2) == FC.reported(m, FC.BAD_LENGTH), f"{what}: bad-record-length bytes"


# ------------------------------------------------------------------ constructed images
def phys(oracle, t, payload):
    """One physical record (db/log_writer.cc:84-115)."""
    crc = oracle.lib.oracle_crc32c_mask(oracle.extend(oracle.extend(0, bytes([t])), payload))
    return struct.pack("<IHB", crc, len(payload), t) + payload


def pay(n, seed=0):
    return bytes((seed + 7 * i) & 0xFF for i in range(n)) if n < 4096 else \
        np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def left(img):
    return BLOCK - len(img) % BLOCK


def fill_block(oracle, img, t=1, seed=0):
    """A record that ends exactly at the block's end."""
    return img + phys(oracle, t, pay(left(img) - HEADER, seed))


def zero_rest(img):
    return img + b"\0" * (left(img) % BLOCK)


def flip(img, at):
    b = bytearray(img)
    b[at] ^= 0x40
    return bytes(b)


@pytest.fixture(scope="module")
def two_blocks(oracle):
    img, _ = log_image([pay(700, k) for k in range(60)] + [pay(40000, 3)], oracle)
    assert len(img) > 2 * BLOCK + 7
    return img


@pytest.mark.parametrize("n", [0, 1, 6, 7, BLOCK, BLOCK + 6, BLOCK + 7])
def test_sizes_around_a_header_and_a_block(ctx, two_blocks, n):
    check_image(ctx, two_blocks[:n], f"intact image cut to {n}")
    check_image(ctx, b"\0" * n, f"{n} zero bytes")
    check_image(ctx, phys_free_header(n), f"{n} bytes of 0xFF")


def phys_free_header(n):
    return b"\xff" * n  # every header has l = 65535: a bad length in a full block, not reported in a short one


def test_block_of_empty_records(ctx, oracle):
    img = phys(oracle, 1, b"") * 4681 + b"\0" + phys(oracle, 1, pay(10))
    assert len(img) == BLOCK + 17 and kvsep.log_walk(img)[0].size == 4682
    check_image(ctx, img, "4,681 empty records and a spare byte")


def test_one_record_fills_a_block(ctx, oracle):
    img = phys(oracle, 1, pay(32761, 5)) + phys(oracle, 2, pay(5))
    assert len(img) == BLOCK + 12
    check_image(ctx, img, "one record of l = 32761")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_trailers(ctx, oracle, k):
    img = phys(oracle, 1, pay(BLOCK - HEADER - k, k)) + b"\0" * k
    img += phys(oracle, 2, pay(20)) + phys(oracle, 4, pay(BLOCK - 27 - HEADER - k, k)) + b"\0" * k + b"\0" * k
    assert len(img) == 2 * BLOCK + k
    check_image(ctx, img, f"trailers of {k} bytes and a last block of {k}")


def many_blocks(oracle, blocks):
    parts = []
    for b in range(blocks):
        if b % 3 == 0:  # a short record, then a zero header: the next live record carries a gap
            blk = zero_rest(phys(oracle, 1, pay(100, b)))
        elif b % 3 == 1:  # two records that fill the block
            blk = fill_block(oracle, phys(oracle, 2, pay(16377, b)), 4, b)
        else:  # a trailer of 3 bytes
            blk = phys(oracle, 1, pay(50, b))
            blk += phys(oracle, 1, pay(BLOCK - len(blk) - HEADER - 3, b)) + b"\0" * 3
        assert len(blk) == BLOCK
        parts.append(blk)
    return b"".join(parts)


@pytest.fixture(scope="module")
def img65(oracle):
    return many_blocks(oracle, 65)


def test_more_blocks_than_a_wave(ctx, img65):
    check_image(ctx, img65, "65 blocks")
    check_image(ctx, flip(flip(img65, 40 * BLOCK + 20), 64 * BLOCK + 9), "65 blocks, two damaged")


def test_more_blocks_than_a_scan_tile(ctx, oracle):
    img = many_blocks(oracle, 1030)
    nrec = kvsep.log_walk(img)[0].size
    check_image(ctx, flip(img, 1025 * BLOCK + 100), "1,030 blocks", caps=[nrec - 1, nrec + 3])


def test_zero_header_in_the_middle_of_a_block(ctx, oracle):
    img = zero_rest(phys(oracle, 1, pay(100)) + phys(oracle, 2, pay(100)))
    img += phys(oracle, 3, pay(50)) + phys(oracle, 4, pay(60))
    img = fill_block(oracle, img)
    check_image(ctx, img, "a zero header in the middle of a block")


def test_bad_length_in_a_full_and_in_a_short_last_block(ctx, oracle):
    a = phys(oracle, 1, pay(100))
    blk = fill_block(oracle, a + phys(oracle, 1, pay(300)) + phys(oracle, 1, pay(300)))
    at = len(a) + 4
    full = blk[:at] + b"\xff\xff" + blk[at + 2:] + phys(oracle, 1, pay(10))
    assert kvsep.log_accept_gaps(full, np.ones(2, np.uint8))[3] == BLOCK - len(a)
    check_image(ctx, full, "a bad length in a full block")
    short = fill_block(oracle, a) + blk[:at] + b"\xff\xff" + blk[at + 2:2000]
    assert kvsep.log_walk(short)[0].size == 3 and kvsep.log_accept_gaps(short, np.ones(3, np.uint8))[3] == 0
    check_image(ctx, short, "a bad length in a short last block")


def six_blocks(oracle, special):
    """Six blocks of four records; special: {(block, record): type}."""
    img = b""
    for b in range(6):
        for r in range(3):
            img += phys(oracle, special.get((b, r), 1), pay(3000, b * 4 + r))
        img = fill_block(oracle, img, special.get((b, 3), 1), b)
    return img


def test_dead_part_of_a_block(ctx, oracle):
    img = six_blocks(oracle, {})
    check_image(ctx, flip(img, 2 * BLOCK + 3007 + 100), "a bad CRC in the middle of a block")


def test_type_5_stops_the_reader(ctx, oracle):
    img = six_blocks(oracle, {(3, 1): 5})
    at = 4 * BLOCK + 3007 + 4
    img = img[:at] + b"\xff\xff" + img[at + 2:]  # a bad length after the stop: uncounted
    img = flip(img, 5 * BLOCK + 50)  # ... and a bad CRC: uncounted
    walk, count, ok, accept, gap, dropped, bad_len = host_expect(img, 10 ** 6)
    assert accept[:13].all() and not accept[13:].any() and (dropped, bad_len) == (0, 0)
    check_image(ctx, img, "a good type 5 in block 3 of 6")


def test_type_5_that_does_not_stop_the_reader(ctx, oracle):
    img = six_blocks(oracle, {(3, 1): 5, (1, 2): 6})
    bad_crc = flip(img, 3 * BLOCK + 3007 + 100)  # the type 5's own payload
    assert host_expect(bad_crc, 10 ** 6)[3][-1] == 1
    check_image(ctx, bad_crc, "a type 5 with a bad CRC, and a type 6")
    dead = flip(img, 3 * BLOCK + 100)  # the record before it: the type 5 lies in the dead part
    assert host_expect(dead, 10 ** 6)[3][-1] == 1
    check_image(ctx, dead, "a type 5 in the dead part of a block")


@pytest.mark.parametrize("tail", [0, 3])
def test_gap_across_all_zero_blocks(ctx, oracle, tail):
    head = fill_block(oracle, phys(oracle, 1, pay(200)))
    head += zero_rest(phys(oracle, 1, pay(100))) + b"\0" * (2 * BLOCK)
    img = head + phys(oracle, 2, pay(100)) + phys(oracle, 4, pay(100))
    img = fill_block(oracle, img)
    img = fill_block(oracle, img + phys(oracle, 1, pay(9)))  # records and no skip: nothing pending after it
    img += phys(oracle, 1, pay(9)) + b"\0" * tail
    gap = host_expect(img, 10 ** 6)[4]
    assert gap.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]  # on the first record three blocks later, nowhere else
    check_image(ctx, img, f"a gap across two all-zero blocks, {tail} bytes after")
    check_image(ctx, head + b"\0" * tail, f"a skip, two all-zero blocks and a final block of {tail} bytes")


@pytest.mark.parametrize("shift", [1, 3])
def test_unaligned_image_between_guard_bytes(ctx, img65, shift):
    check_image(ctx, flip(img65[:3 * BLOCK + 1000], BLOCK + 30), f"image at base + {shift}", shift=shift)


def test_callers_own_stream(ctx, img65):
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    check_image(ctx, img65[:5 * BLOCK + 77], "a caller's own stream", stream=s)


# ------------------------------------------------------------------ the accept pass alone
@pytest.mark.parametrize("verdicts", ["ones", "zeros", "one zero per block"])
def test_accept_gaps_device_on_written_verdicts(ctx, img65, verdicts):
    off, ln, stored, ty = kvsep.log_walk(img65)
    nrec = off.size
    ok = np.ones(nrec, np.uint8)
    if verdicts == "zeros":
        ok[:] = 0
    elif verdicts == "one zero per block":
        blk = (off // np.uint64(BLOCK)).astype(np.int64)
        for i in range(1, nrec):  # the second record of every block that has one, and the only one of block 0
            if blk[i] == blk[i - 1] and (i < 2 or blk[i - 2] != blk[i]):
                ok[i] = 0
        ok[0] = 0
    d = upload(img65)
    for cap in (nrec - 1, nrec, nrec + 3):
        count = min(nrec, cap)
        accept, gap, dropped, bad_len = kvsep.log_accept_gaps(img65, ok[:count])
        a = Arrays(cap)
        a.p("off")[:count] = torch.from_numpy(off[:count].view(np.int64)).to(DEV)
        a.p("len")[:count] = torch.from_numpy(ln[:count].view(np.int64)).to(DEV)
        a.p("type")[:count] = torch.from_numpy(ty[:count]).to(DEV)
        a.p("ok")[:count] = torch.from_numpy(ok[:count]).to(DEV)
        a.words[0] = nrec
        ctx.log_accept_gaps_device(d.data_ptr(), len(img65), a.p("off"), a.p("len"), a.p("type"), a.p("ok"),
                                   a.words[0:1], a.p("accept"), gap=a.p("gap"), dropped=a.words[1:2],
                                   bad_length=a.words[2:3], cap=cap)
        torch.cuda.synchronize()
        assert np.array_equal(a.get("accept", np.uint8), padded(accept, cap, np.uint8)), (verdicts, cap)
        assert np.array_equal(a.get("gap", np.uint8), padded(gap, cap, np.uint8)), (verdicts, cap)
        assert (a.word(1), a.word(2)) == (dropped, bad_len), (verdicts, cap)
        # without the nullable outputs: accept alone
        b = Arrays(cap)
        ctx.log_accept_gaps_device(d.data_ptr(), len(img65), a.p("off"), a.p("len"), a.p("type"), a.p("ok"),
                                   a.words[0:1], b.p("accept"), cap=cap)
        torch.cuda.synchronize()
        assert np.array_equal(b.get("accept", np.uint8), padded(accept, cap, np.uint8)), (verdicts, cap)
        assert (b.get("gap", np.uint8) == S8).all() and b.word(1) == S64 & 0xFFFFFFFFFFFFFFFF


def test_refusals(ctx):
    a = Arrays(4)
    d = upload(b"\0" * 64)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null base"):
        ctx.log_walk_device(0, 64, a.words[0:1], off=a.p("off"), cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null nrec"):
        ctx.log_walk_device(d.data_ptr(), 64, None, off=a.p("off"), cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*2\^32"):
        ctx.log_walk_device(d.data_ptr(), 64, a.words[0:1], off=a.p("off"), cap=1 << 32)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null"):
        ctx.log_accept_gaps_device(d.data_ptr(), 64, a.p("off"), a.p("len"), a.p("type"), a.p("ok"), a.words[0:1],
                                   None, cap=4)
    with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*null"):
        ctx.log_read_device(d.data_ptr(), 64, a.p("off"), a.p("len"), None, a.p("type"), a.p("ok"), a.p("accept"),
                            a.words[0:1], cap=4)
    torch.cuda.synchronize()
    assert (a.words.cpu().numpy() == S64).all()


# ------------------------------------------------------------------ capture
def test_captured_read_follows_each_replay(img65):
    """reserve, then walk -> checksum -> accept in one graph; the image is rewritten in place between replays."""
    intact = img65[:9 * BLOCK + 500]
    damaged = flip(intact, 2 * BLOCK + 40)  # the first record of block 2: the block is dead from its start
    at = 4 * BLOCK + 4
    damaged = damaged[:at] + b"\xff\xff" + damaged[at + 2:]  # a bad length where block 4's first record stood
    n, nb = len(intact), 10
    cap = kvsep.log_walk(intact)[0].size + 3
    c = kvsep.Context(0)
    try:
        d = upload(intact)
        a = Arrays(cap)
        c.reserve(max(cap, nb), n)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.log_read_device(d.data_ptr(), n, a.p("off"), a.p("len"), a.p("stored"), a.p("type"), a.p("ok"),
                              a.p("accept"), a.words[0:1], gap=a.p("gap"), dropped=a.words[1:2],
                              bad_length=a.words[2:3], cap=cap, stream=torch.cuda.current_stream())
        assert c.capture_sets()[1] == 1
        for img in (intact, damaged, intact):
            d[:n] = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(DEV)
            g.replay()
            torch.cuda.synchronize()
            walk, count, ok, accept, gap, dropped, bad_len = host_expect(img, cap)
            assert a.word(0) == walk[0].size
            for name, w, dt in (("off", walk[0], np.uint64), ("len", walk[1], np.uint64),
                                ("stored", walk[2], np.uint32), ("type", walk[3], np.uint8), ("ok", ok, np.uint8),
                                ("accept", accept, np.uint8), ("gap", gap, np.uint8)):
                assert np.array_equal(a.get(name, dt), padded(w, cap, dt)), name
            assert (a.word(1), a.word(2)) == (dropped, bad_len)
        assert host_expect(damaged, cap)[5] > 0 and host_expect(damaged, cap)[6] > 0
        # larger than the reservation: refused at capture, nothing enqueued
        big = Arrays(max(cap, nb) + 1)
        wide = upload(b"\0" * ((max(cap, nb) + 1) * BLOCK))
        torch.cuda.synchronize()
        for kw in (dict(n=n, arr=big), dict(n=(max(cap, nb) + 1) * BLOCK, arr=a)):
            arr = kw["arr"]
            arr.words.fill_(S64)
            torch.cuda.synchronize()
            with pytest.raises(kvsep.KvsepError, match=r"\(-1\).*reserve"):
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2):
                    c.log_read_device(wide.data_ptr(), kw["n"], arr.p("off"), arr.p("len"), arr.p("stored"),
                                      arr.p("type"), arr.p("ok"), arr.p("accept"), arr.words[0:1], gap=arr.p("gap"),
                                      cap=arr.cap, stream=torch.cuda.current_stream())
            del g2
            torch.cuda.synchronize()
            assert (arr.words.cpu().numpy() == S64).all()
        del g
        c.release_captures()
    finally:
        c.close()
