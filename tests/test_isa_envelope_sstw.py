"""The memory envelope of the SST table writer's kernels: the shipped gfx950 assembly reads and writes exactly what
crc32c_sstbuild.inc and the public header promise, and a replay reads no scratch word it did not write.  CPU only.

tests/test_isa_envelope_sst.py does this for the table reader; this file runs, under tools/wave_emu.py and with
test_isa_envelope_framing.py's Call (one call's emulated memory and its checks),

  crc32c_sstbuild.inc   sst_keys_count / sst_keys_fill / sstw_size / sstw_fill / sstw_tail / sstw_keep

with the stop kernel and the offsets kernels between them, as the whole stream-ordered chains of
kvsep_sst_index_keys_device, kvsep_sst_index_build_device and kvsep_sst_table_finish_device in one emulated Memory.  The
builder's one CRC call is not run here (tests/test_isa_envelope.py covers the CRC kernels): the harness reads the
position and length the fill kernel posted, computes the checksum by the library's host leg and puts it where the CRC
kernel would.  Grids, block sizes and scratch slices come from tests/cpp/sstw_geometry.cc.  Per run:

 a. reads: every caller array is a region of exactly its documented length (key_off / key_len / blk_off / blk_len count
    words, keep count bytes, the position one word; an empty one is an unmapped address); the key source sits in a guard
    region at a skew past a 4 KiB boundary with no slack behind it and is read only for kept entries: bytewise inside
    their keys where the wave stages its range, inside the naturally aligned 16-B granules that hold such a byte where
    the range is over the staging area; after a refusal it is not read at all;
 b. writes: dst is a region of exactly dst_bytes and carries a write mark on exactly the bytes of the block and its
    trailer (the table form: the metaindex block, the index block, both trailers, the footer) and on none after a
    refusal; *out_len, *status and *table_bytes on every byte; nothing else but the scratch is written;
 c. replay soundness: the builder's scratch, the walk's and the offsets pass's are filled with 0xA5 and declared
    scratch: no read of a scratch byte that this call has not stored;
 d. results: equal to the host forms kvsep.sst_index_build / sst_footer_build / sst_index_keys.
"""
import os
import subprocess

import numpy as np
import pytest

import sst_tables as T
import test_isa_envelope_framing as F

env = F.env
CSRC, ROOT, ASM, M64 = F.CSRC, F.ROOT, F.ASM, F.M64

K = {"sst_keys_count": "_ZN5kvsep21sst_keys_count_kernelENS_12SstIndexArgsE",
     "sst_keys_fill": "_ZN5kvsep20sst_keys_fill_kernelENS_11SstKeysArgsE",
     "sstw_size": "_ZN5kvsep16sstw_size_kernelENS_12SstBuildArgsE",
     "sstw_fill": "_ZN5kvsep16sstw_fill_kernelENS_12SstBuildArgsE",
     "sstw_tail": "_ZN5kvsep16sstw_tail_kernelENS_12SstBuildArgsE",
     "sstw_keep": "_ZN5kvsep16sstw_keep_kernelEPKhPKyPKjmPh",
     "sst_index_stop": "_ZN5kvsep21sst_index_stop_kernelEPKymS1_Py",
     "offsets_tile_sum": F.K["offsets_tile_sum"], "offsets_tile_scan": F.K["offsets_tile_scan"],
     "offsets_write": F.K["offsets_write"]}
STRUCTS = {"SstIndexArgs": "crc32c_sstindex.inc", "SstBuildArgs": "crc32c_sstbuild.inc",
           "OffsetsArgs": "crc32c_offsets.inc"}


class Geometry:
    def __init__(self, tmp):
        self.exe = os.path.join(tmp, "sstw_geometry")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                               os.path.join(ROOT, "tests", "cpp", "sstw_geometry.cc"), "-o", self.exe])
        self.const = self.pairs("constants")

    def ask(self, *args):
        return subprocess.check_output([self.exe] + [str(a) for a in args], text=True).splitlines()

    def pairs(self, *args):
        return {k: int(v) for k, v in (ln.split() for ln in self.ask(*args))}

    def kernels(self, *args):
        return [(k[:-len("_kernel")], int(g), int(t)) for k, g, t in (ln.split() for ln in self.ask(*args))]


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    return Geometry(str(tmp_path_factory.mktemp("sstw_geometry")))


class Call(F.Call):
    """F.Call with this file's kernel names and structs."""

    def launch(self, kernel, grid, threads, args):
        if grid == 0:
            return
        try:
            self.steps += self.E.launch_args(self.mem, ASM, K[kernel], threads, args, grid)
        except self.E.EmuError as e:
            raise AssertionError("%s: %s: %s\n  arrays: %s" % (
                self.tag, kernel, e, ", ".join("%s@0x%x+%d" % (n, a, self.size[n]) for n, a in self.addr.items()))) from e

    def sargs(self, kernel, struct, values):
        return self.E.struct_kernarg(ASM, K[kernel], os.path.join(CSRC, STRUCTS[struct]), struct, values)

    def pargs(self, kernel, values):
        return self.E.args_kernarg(ASM, K[kernel], values)

    def keys_args(self, kernel, values, key_off, key_len):
        """SstKeysArgs: an SstIndexArgs and the two key arrays behind it; the size is checked against the metadata."""
        fields = self.E.struct_fields(os.path.join(CSRC, STRUCTS["SstIndexArgs"]), "SstIndexArgs")
        inner = fields["sizeof"][0]
        explicit = [a for a in self.E.kernel_args(ASM, K[kernel]) if not a[2].startswith("hidden_")]
        assert len(explicit) == 1 and explicit[0][1] == inner + 16, explicit
        img = bytearray(inner + 16)
        for k, v in values.items():
            o, size = fields[k]
            img[o:o + size] = int(v).to_bytes(size, "little")
        img[inner:inner + 8] = int(key_off).to_bytes(8, "little")
        img[inner + 8:] = int(key_len).to_bytes(8, "little")
        return bytes(img)

    def written(self, name):
        return self.mem.touched(self.addr[name])[2]


def offsets_values(sizes, d_tile, d_ext, seg_len, count, dst_off, end, keep_before=0):
    return dict(seg_len=seg_len, keep_before=keep_before, max_size=M64, count=count, nseg=count, dst_off=dst_off, end=end,
                ext=d_ext, **{k: d_tile + 8 * sizes[k] for k in ("tile_sum", "tile_kept", "tile_base", "grand")})


# ------------------------------------------------------------------------------------------------- the builder
def entry_size(kl, bo, bl):
    val = T.handle_bytes(bo, bl)
    return len(T.varint(0) + T.varint(kl) + T.varint(len(val))) + kl + len(val)


def run_build(env, geo, tag, count, at, key_skew, table, long_key=False, short=0):
    """One kvsep_sst_index_build_device (table: kvsep_sst_table_finish_device) over `count` entries; short: bytes that
    dst lacks (a refusal)."""
    import kvsep
    rng = np.random.default_rng(count * 31 + at)
    kl = np.full(count, 21, np.uint64)
    if count > 2:
        kl[1], kl[2] = 0, 130
    if long_key and count > 3:
        kl[3] = geo.const["kStageBytes"] + 5
    gaps = rng.integers(0, 19, count).astype(np.uint64)
    ko = (np.cumsum(kl + gaps) - kl).astype(np.uint64) if count else np.zeros(0, np.uint64)
    src = rng.integers(0, 256, int(ko[-1] + kl[-1]) if count else 1, dtype=np.uint8)
    keep = (np.arange(count) % 3 != 1).astype(np.uint8)
    if count > 2:
        keep[1] = keep[2] = 1
    bo = (np.arange(count, dtype=np.uint64) * 4101).astype(np.uint64)
    bo[5::7] = M64  # a block the salvage did not lay out
    bl = (4096 + np.arange(count) % 200).astype(np.uint64)
    kept = [i for i in range(count) if keep[i] and int(bo[i]) != M64]

    block, want_len, st = kvsep.sst_index_build(src, ko, kl, bo, bl, keep=keep)
    assert st == kvsep.SSTW_OK and len(block) == want_len + 5
    if table:
        meta = kvsep.sst_index_build(b"", [], [], [], [])[0]
        want = meta + block + kvsep.sst_footer_build((at, 8), (at + 13, want_len))
    else:
        want = block
    dst_bytes = at + len(want) - short
    refused = short > 0

    c = Call(env, tag)
    d_src = c.image(src, key_skew)
    sizes = geo.pairs("scratch", count)
    d_w = c.scratch("sstw", 8 * sizes["total"])
    d_ext = c.scratch("ext", 8 * count)
    d_tile = c.scratch("tile", 8 * sizes["tile_words"])
    words = d_w + 8 * sizes["words"]
    word = lambda k: words + 8 * geo.const[k]
    d_dst = c.output("dst", dst_bytes)
    v = dict(key_base=d_src, key_off=c.input("key_off", ko), key_len=c.input("key_len", kl),
             blk_off=c.input("blk_off", bo), blk_len=c.input("blk_len", bl), keep=c.input("keep", keep), count=count,
             dst=d_dst, dst_bytes=dst_bytes, at=c.input("at", np.array([at], np.uint64)),
             lead=geo.const["kMetaFramed"] if table else 0, trail=geo.const["kFooter"] if table else 0, source=0,
             size=d_w + 8 * sizes["size"], flag=d_w + 8 * sizes["flag"], pos=d_w + 8 * sizes["pos"],
             rank=d_w + 8 * sizes["rank"], words=words, out_len=c.output("out_len", 8), status=c.output("status", 4),
             table_bytes=c.output("table_bytes", 8) if table else 0,
             meta_masked=int.from_bytes(T.trailer(T.index_block([], []))[1:], "little"),
             tabs=c.input("tabs", np.frombuffer(env.tables(), np.uint8)))
    passes = [offsets_values(sizes, d_tile, d_ext, v["size"], count, v["pos"], word("kEntriesBytes")),
              offsets_values(sizes, d_tile, d_ext, v["flag"], count, v["rank"], word("kNKept"))]
    nt = (count + 1023) // 1024
    done = 0
    for kernel, grid, threads in geo.kernels("build", count):
        if kernel == "offsets_tile_scan":
            ov = passes[done]
            c.launch(kernel, grid, threads, c.pargs(kernel, [ov["tile_sum"], ov["tile_kept"], ov["tile_base"],
                                                            ov["grand"], nt]))
        elif kernel.startswith("offsets"):
            c.launch(kernel, grid, threads, c.sargs(kernel, "OffsetsArgs", passes[done]))
            done += kernel == "offsets_write"
        else:
            if kernel == "sstw_tail":
                # the CRC call over the one block the fill kernel posted, by the library's host leg; its store of the
                # result counts as the call's own
                o, k = c.mem.peek64(word("kCrcOff")), c.mem.peek64(word("kCrcLen"))
                assert (o, k) == ((0, 0) if refused else (at + v["lead"], want_len)), tag
                crc = kvsep.value(c.get("dst", np.uint8)[o:o + k].tobytes())
                c.mem.view(word("kCrc"), 4).view(np.uint32)[0] = crc
                c.mem.scratch[d_w][word("kCrc") - d_w:word("kCrc") - d_w + 4] = True
            c.launch(kernel, grid, threads, c.sargs(kernel, "SstBuildArgs", v))

    # ---- (d) and (b)
    got = int(c.get("out_len", np.uint64)[0]), int(c.get("status", np.uint32)[0])
    assert got == (want_len, kvsep.SSTW_NO_ROOM if refused else kvsep.SSTW_OK), "%s: (*out_len, *status) = %s" % (tag, got)
    if table:
        assert int(c.get("table_bytes", np.uint64)[0]) == (0 if refused else at + len(want)), tag
    wr = c.written("dst")
    expect = np.zeros(dst_bytes, bool)
    if not refused:
        expect[at:] = True
        assert c.get("dst", np.uint8)[at:].tobytes() == want, tag + ": dst differs from the host form"
    diff = np.nonzero(wr != expect)[0]
    assert not diff.size, "%s: dst write marks differ from the block's bytes at %s" % (tag, diff[:8])
    # ---- (a) the key source
    region, pay, n = c.img
    _, rd, _ = c.mem.touched(region)
    allowed = np.zeros(rd.size + 16, bool)
    if not refused:
        for w0 in range(0, count, 64):
            mine = [i for i in kept if w0 <= i < w0 + 64]
            staged = sum(entry_size(int(kl[i]), int(bo[i]), int(bl[i])) for i in mine) <= geo.const["kStageBytes"]
            for i in mine:
                a, e = pay + int(ko[i]), pay + int(ko[i]) + int(kl[i])
                if e > a:
                    lo, hi = (a, e) if staged else (a // 16 * 16, -(-e // 16) * 16)
                    allowed[lo - region:hi - region] = True
    bad = np.nonzero(rd & ~allowed[:rd.size])[0]
    assert not bad.size, "%s: key source read at offset %d, outside the kept keys" % (tag, int(bad[0]) - (pay - region))
    if long_key and not refused and count > 3:
        assert rd.any()
    for name, size in (("blk_off", 8), ("keep", 1)):  # the keep rule looks at every entry
        assert c.reads(name, size).all(), "%s: %s not read in full" % (tag, name)
    for name in ("key_len", "blk_len", "key_off"):  # ... a dropped entry's key and length need not be looked at
        assert c.reads(name, 8)[kept].all() or refused and name == "key_off", "%s: %s of a kept entry not read" % (tag, name)
    c.check(partial_out=("dst",), granule_image=True)


@pytest.mark.parametrize("count,at,key_skew,table", [
    (0, 0, 0, False), (0, 1, 1, True), (1, 15, 4095, False), (1, 16, 15, True), (65, 0, 1, True), (65, 1, 0, False),
    (65, 15, 4095, False), (65, 16, 15, True), (1025, 1, 4095, False), (1025, 16, 0, True)])
def test_build(env, geo, count, at, key_skew, table):
    run_build(env, geo, "sstw %s %d at %d key skew %d" % ("finish" if table else "build", count, at, key_skew), count,
              at, key_skew, table)


@pytest.mark.parametrize("at,key_skew,table", [(0, 15, False), (1, 1, True), (15, 0, False), (16, 4095, True)])
def test_build_with_a_key_over_the_staging_area(env, geo, at, key_skew, table):
    """One key over sstw::kStageBytes: its wave writes entry by entry, the key as a pack span (granule reads)."""
    run_build(env, geo, "sstw long key at %d key skew %d%s" % (at, key_skew, " table" if table else ""), 65, at,
              key_skew, table, long_key=True)


@pytest.mark.parametrize("count,table", [(0, False), (65, True), (65, False)])
def test_build_refused_writes_nothing(env, geo, count, table):
    run_build(env, geo, "sstw no room %d%s" % (count, " table" if table else ""), count, 15, 1, table, short=1)


# ------------------------------------------------------------------------------------------------- the keys walk
def run_keys(env, geo, tag, img, index, cap, runs, skew):
    import kvsep
    img = np.ascontiguousarray(np.frombuffer(bytes(img), np.uint8))
    n = img.size
    ioff, ilen = index
    c = Call(env, tag)
    d_img = c.image(img, skew)
    sizes = geo.pairs("walk_scratch", runs)
    nt, nwg = sizes["tiles"], sizes["workgroups"]
    d_idx = c.scratch("sstidx", 8 * sizes["words"])
    d_ext = c.scratch("ext", 8 * runs)
    d_tile = c.scratch("tile", 8 * sizes["tile_words"])
    outs = {k: c.output(k, 8 * cap) for k in ("off", "len", "key_off", "key_len")}
    d_nb, d_st = c.output("nblocks", 8), c.output("status", 4)
    stop, cnt = d_idx, d_idx + 8 * geo.const["kStopWords"]
    errbase, wgstop = cnt + 8 * runs, cnt + 16 * runs
    wv = dict(img=d_img, n=n, handle=c.input("handle", np.array(index, np.uint64)), runs=runs, off=outs["off"],
              len=outs["len"], cap=cap, nblocks=d_nb, status=d_st, stop=stop, cnt=cnt, errbase=errbase, wgstop=wgstop)
    ov = offsets_values(sizes, d_tile, d_ext, cnt, runs, errbase, d_nb, keep_before=stop)
    for kernel, grid, threads in geo.kernels("keys", runs, cap):
        if kernel == "sst_index_stop":
            c.launch(kernel, grid, threads, c.pargs(kernel, [wgstop, nwg, errbase, stop]))
        elif kernel == "offsets_tile_scan":
            c.launch(kernel, grid, threads, c.pargs(kernel, [ov["tile_sum"], ov["tile_kept"], ov["tile_base"],
                                                            ov["grand"], nt]))
        elif kernel.startswith("offsets"):
            c.launch(kernel, grid, threads, c.sargs(kernel, "OffsetsArgs", ov))
        elif kernel == "sst_keys_fill":
            c.launch(kernel, grid, threads, c.keys_args(kernel, wv, outs["key_off"], outs["key_len"]))
        else:
            c.launch(kernel, grid, threads, c.sargs(kernel, "SstIndexArgs", wv))
    w_off, w_len, w_ko, w_kl, want_n, want_status = kvsep.sst_index_keys(img[ioff:ioff + ilen].tobytes(), cap=cap)
    m = min(want_n, cap)
    w_ko = w_ko.copy()
    w_ko[:m] += np.uint64(ioff)  # the device form's offsets are the image's
    got = int(c.get("nblocks", np.uint64)[0]), int(c.get("status", np.uint32)[0])
    assert got == (want_n, want_status), "%s: (*nblocks, *status) = %s, the host form gives %s" % (
        tag, got, (want_n, want_status))
    for name, want in (("off", w_off), ("len", w_len), ("key_off", w_ko), ("key_len", w_kl)):
        assert np.array_equal(c.get(name, np.uint64), want), "%s: %s" % (tag, name)
    base, rd, _ = c.mem.touched(d_img)
    lo = d_img - base
    stray = rd.copy()
    stray[lo + ioff:lo + ioff + ilen] = False
    assert not stray.any(), "%s: image read at offset %d, outside the index block" % (
        tag, int(np.nonzero(stray)[0][0]) - lo)
    c.check(granule_image=True)
    return want_n, want_status


@pytest.mark.parametrize("nblocks,interval,skew,cap_delta,spare", [
    (0, 1, 0, 0, 0), (1, 1, 1, 0, 2), (65, 1, 4095, -1, 3), (65, 1, 15, 3, 200), (65, 2, 1, 0, 0), (300, 1, 4095, 0, 1)])
def test_keys_walk(env, geo, nblocks, interval, skew, cap_delta, spare):
    import kvsep
    img, off, ln, meta, index = T.build_table(nblocks, interval, block_len=lambda i: 9 + i % 7, seed=3)
    nr = int.from_bytes(img[index[0] + index[1] - 4:index[0] + index[1]].tobytes(), "little")
    got = run_keys(env, geo, "sst keys %d/%d skew %d cap%+d runs+%d" % (nblocks, interval, skew, cap_delta, spare), img,
                   index, max(nblocks + cap_delta, 0), nr + spare, skew)
    assert got == ((1, kvsep.SST_SHARED_KEY) if interval == 2 else (nblocks, kvsep.SST_OK))


# ------------------------------------------------------------------------------------------------- the keep mask
@pytest.mark.parametrize("cap,nblocks,status", [(2, 0, 0), (67, 65, 0), (67, 65, 8), (67, 80, 7), (300, 3, 2),
                                                (1030, 1025, 5)])
def test_keep_mask(env, geo, cap, nblocks, status):
    tag = "sstw keep cap %d nblocks %d status %d" % (cap, nblocks, status)
    ok = (np.arange(cap) % 5 != 2).astype(np.uint8)
    c = Call(env, tag)
    args = [c.input("ok", ok), c.input("nblocks", np.array([nblocks], np.uint64)),
            c.input("status", np.array([status], np.uint32)), cap, c.output("keep", cap)]
    for kernel, grid, threads in geo.kernels("keep", cap):
        c.launch(kernel, grid, threads, c.pargs(kernel, args))
    want = ok.copy()
    want[min(nblocks, cap - 2):] = 0
    if status in (1, 2, 3, 8):
        want[:] = 0
    assert np.array_equal(c.get("keep", np.uint8), want), tag
    c.check()


def test_every_kernel_of_the_file_is_run():
    """The kernels of crc32c_sstbuild.inc are the ones named here: none is skipped."""
    import re
    src = open(os.path.join(CSRC, "crc32c_sstbuild.inc")).read()
    names = set(re.findall(r"\b(sstw?_[a-z_]+)_kernel\(", re.sub(r"//.*", "", src)))
    assert names == {k for k in K if k.startswith(("sstw_", "sst_keys"))}, names
