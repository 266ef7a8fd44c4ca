"""The memory envelope of the SST table reader's kernels: the shipped gfx950 assembly reads and writes exactly what
crc32c_sstindex.inc and the public header promise, and a replay reads no scratch word it did not write.  CPU only.

tests/test_isa_envelope_framing.py does this for the framing, layout and log kernels; this file runs, under
tools/wave_emu.py and with that file's Call (one call's emulated memory and its checks),

  crc32c_sstindex.inc   sst_footer / sst_index_count / sst_index_stop / sst_index_fill / sst_table_prep

and the three offsets kernels between stop and fill -- the walk alone (kvsep_sst_index_device) and the table form
(kvsep_sst_table_verify_device) as their whole stream-ordered chains in one emulated Memory.  The table form's two CRC
calls are not run here (tests/test_isa_envelope.py covers the CRC kernels): the checksum word the walk's count kernel
reads from crc[0] is put there by the harness, computed by the library's host leg.  The grids, block sizes and the
scratch size come from tests/cpp/sst_geometry.cc, a host program over the pure headers the launch code uses.  Per run:

 a. reads: every caller array is a region of exactly its documented length (handle 2 words, handles 4, off / len cap
    elements, crc cap words, nblocks one word, status one word); the image sits in a guard region at 0, 1, 15 or 4095
    bytes past a 4 KiB boundary with no slack behind it and is read bytewise, only inside the footer, the index block
    with its type byte, and the 4-byte stored words of the listed handles that are usable -- never written;
 b. writes: off / len carry a write mark on every byte of their cap elements, nblocks, status (and handles) on every
    byte, the SST arrays len1 / stored on every byte of their cap elements; nothing else but the scratch is written;
 c. replay soundness: the walk's scratch, the offsets pass's and the SST arrays are filled with 0xA5 and declared
    scratch: no read of a scratch byte that this call has not stored;
 d. results: equal to the host forms kvsep.sst_footer / kvsep.sst_index_walk, the slot layout built from them, and the
    read check's lengths and stored words restated here.
"""
import numpy as np
import pytest

import sst_tables as T
import test_isa_envelope_framing as F

import os

env = F.env  # the module fixture that builds the assembly and loads the emulator
CSRC, ROOT, ASM, M64 = F.CSRC, F.ROOT, F.ASM, F.M64

K = {"sst_footer": "_ZN5kvsep17sst_footer_kernelEPKhmPmPj",
     "sst_index_count": "_ZN5kvsep22sst_index_count_kernelENS_12SstIndexArgsE",
     "sst_index_stop": "_ZN5kvsep21sst_index_stop_kernelEPKymS1_Py",
     "sst_index_fill": "_ZN5kvsep21sst_index_fill_kernelENS_12SstIndexArgsE",
     "sst_table_prep": "_ZN5kvsep21sst_table_prep_kernelENS_11SstPrepArgsE",
     "offsets_tile_sum": F.K["offsets_tile_sum"], "offsets_tile_scan": F.K["offsets_tile_scan"],
     "offsets_write": F.K["offsets_write"]}
STRUCTS = {"SstIndexArgs": "crc32c_sstindex.inc", "SstPrepArgs": "crc32c_sstindex.inc",
           "OffsetsArgs": "crc32c_offsets.inc"}


class Geometry:
    def __init__(self, tmp):
        import subprocess
        self.exe = os.path.join(tmp, "sst_geometry")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                               os.path.join(ROOT, "tests", "cpp", "sst_geometry.cc"), "-o", self.exe])
        self.const = self.pairs("constants")

    def ask(self, *args):
        import subprocess
        return subprocess.check_output([self.exe] + [str(a) for a in args], text=True).splitlines()

    def pairs(self, *args):
        return {k: int(v) for k, v in (ln.split() for ln in self.ask(*args))}

    def kernels(self, *args):
        """[(kernel, grid, threads)] in stream order."""
        return [(k[:-len("_kernel")], int(g), int(t)) for k, g, t in (ln.split() for ln in self.ask(*args))]


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    return Geometry(str(tmp_path_factory.mktemp("sst_geometry")))


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

    def poke32(self, name, index, value):
        """The harness's own store (the result of a step that is not emulated here): no mark."""
        self.mem.view(self.addr[name] + 4 * index, 4).view(np.uint32)[0] = value

    def written(self, name):
        return self.mem.touched(self.addr[name])[2]


def usable(off, ln, n):
    return off + ln + 5 <= n


def run(env, geo, tag, img, cap, runs, skew, table, index=None, crc_ok=True):
    """One call over the image `img`: the walk alone over the index block `index` = (off, len), or the table form."""
    import kvsep
    img = np.ascontiguousarray(np.frombuffer(bytes(img), np.uint8))
    n = img.size
    c = Call(env, tag)
    d_img = c.image(img, skew)
    sizes = geo.pairs("scratch", runs)
    nt, nwg = sizes["tiles"], sizes["workgroups"]
    d_idx = c.scratch("sstidx", 8 * sizes["words"])
    d_ext = c.scratch("ext", 8 * runs)
    d_tile = c.scratch("tile", 8 * sizes["tile_words"])
    d_off, d_len = c.output("off", 8 * cap), c.output("len", 8 * cap)
    d_nb, d_st = c.output("nblocks", 8), c.output("status", 4)
    stop, cnt = d_idx, d_idx + 8 * geo.const["kStopWords"]
    errbase, wgstop = cnt + 8 * runs, cnt + 16 * runs
    kernels = geo.kernels("table" if table else "walk", runs, cap)
    allowed = np.zeros(n, bool)  # the image bytes this call may read

    if table:
        d_handles = c.output("handles", 32)
        d_crc = c.input("crc", np.zeros(cap, np.uint32))
        d_len1, d_stored = c.scratch("len1", 8 * cap), c.scratch("stored", 4 * cap)
        (moff, mlen, ioff, ilen), fstatus = kvsep.sst_footer(img)
        if n >= geo.const["kFooter"]:
            allowed[n - geo.const["kFooter"]:] = True
        d_handle = d_handles + 16
    else:
        ioff, ilen = index
        fstatus = 0 if usable(ioff, ilen, n) else kvsep.SST_BAD_FOOTER
        d_handle = c.input("handle", np.array(index, np.uint64))
        d_handles = d_crc = d_stored = 0
    if not fstatus:
        allowed[ioff:ioff + ilen + (1 if table else 0)] = True

    wv = dict(img=d_img, n=n, handle=d_handle, runs=runs, handles=d_handles, crc=d_crc, stored=d_stored, off=d_off,
              len=d_len, cap=cap, nblocks=d_nb, status=d_st, stop=stop, cnt=cnt, errbase=errbase, wgstop=wgstop)
    ov = dict(seg_len=cnt, keep_before=stop, max_size=M64, count=runs, nseg=runs, dst_off=errbase, end=d_nb, ext=d_ext,
              **{k: d_tile + 8 * sizes[k] for k in ("tile_sum", "tile_kept", "tile_base", "grand")})
    preps = 0
    for kernel, grid, threads in kernels:
        if kernel == "sst_footer":
            c.launch(kernel, grid, threads, c.pargs(kernel, [d_img, n, d_handles, d_st]))
            got = c.get("handles", np.uint64).tolist(), int(c.get("status", np.uint32)[0])
            assert got == ([moff, mlen, ioff, ilen], fstatus), "%s: the footer kernel gives %s" % (tag, got)
        elif kernel == "sst_table_prep" and preps == 0:
            preps = 1
            c.launch(kernel, grid, threads, c.sargs(kernel, "SstPrepArgs", dict(
                img=d_img, n=n, off=d_handles + 16, len=d_handles + 24, count=1, nblocks=0, status=d_st, cap=cap,
                len1=d_len1, stored=d_stored)))
            # the CRC call over that one slot, by the library's host leg
            if not fstatus:
                allowed[ioff + ilen + 1:ioff + ilen + 5] = True
                assert int(c.mem.peek64(d_len1)) == ilen + 1, tag
                crc = kvsep.value(img[ioff:ioff + ilen + 1].tobytes())
                c.poke32("crc", 0, crc if crc_ok else crc ^ 0x10)
            else:
                assert int(c.mem.peek64(d_len1)) == 0, tag
        elif kernel == "sst_table_prep":
            c.launch(kernel, grid, threads, c.sargs(kernel, "SstPrepArgs", dict(
                img=d_img, n=n, off=d_off, len=d_len, count=cap, nblocks=d_nb, status=d_st, cap=cap, len1=d_len1,
                stored=d_stored)))
        elif kernel == "sst_index_stop":
            c.launch(kernel, grid, threads, c.pargs(kernel, [wgstop, nwg, errbase, stop]))
        elif kernel == "offsets_tile_scan":
            c.launch(kernel, grid, threads, c.pargs(kernel, [ov["tile_sum"], ov["tile_kept"], ov["tile_base"],
                                                            ov["grand"], nt]))
        elif kernel.startswith("offsets"):
            c.launch(kernel, grid, threads, c.sargs(kernel, "OffsetsArgs", ov))
        else:
            c.launch(kernel, grid, threads, c.sargs(kernel, "SstIndexArgs", wv))

    # ---- (d) against the host forms
    block = img[ioff:ioff + ilen].tobytes() if not fstatus else b""
    nr = int.from_bytes(block[-4:], "little") if len(block) >= 4 else 0
    if fstatus:
        want_n, want_status, w_off, w_len = 0, fstatus, [], []
    elif table and not crc_ok:
        want_n, want_status, w_off, w_len = 0, kvsep.SST_INDEX_CHECKSUM, [], []
    elif table and img[ioff + ilen]:
        want_n, want_status, w_off, w_len = 0, kvsep.SST_INDEX_COMPRESSED, [], []
    elif len(block) >= 4 and nr <= (len(block) - 4) // 4 and nr > runs:
        want_n, want_status, w_off, w_len = 0, kvsep.SST_BAD_RESTARTS, [], []  # more runs than the scratch holds
    else:
        w_off, w_len, want_n, want_status = kvsep.sst_index_walk(block)
        w_off, w_len = w_off.tolist(), w_len.tolist()
    room = cap - 2 if table else cap
    m = min(want_n, room)
    slots = list(zip(w_off[:m], w_len[:m]))
    if table:
        slots += [(moff, mlen), (ioff, ilen)]
        if not want_status and want_n + 2 > cap:
            want_status = kvsep.SST_CAP
    listed = 0 if fstatus else len(slots)
    slots += [(0, 0)] * (cap - len(slots))
    got = int(c.get("nblocks", np.uint64)[0]), int(c.get("status", np.uint32)[0])
    assert got == (want_n, want_status), "%s: (*nblocks, *status) = %s, the host forms give %s" % (
        tag, got, (want_n, want_status))
    assert c.get("off", np.uint64).tolist() == [s[0] for s in slots], tag
    assert c.get("len", np.uint64).tolist() == [s[1] for s in slots], tag
    if table:
        exp1, exps = [], []
        for i, (o, k) in enumerate(slots):
            if i >= listed:
                exp1.append(0), exps.append(geo.const["kMaskOfZero"])
            elif not usable(o, k, n):
                exp1.append(0), exps.append(geo.const["kNoMatch"])
            else:
                exp1.append(k + 1), exps.append(int.from_bytes(img[o + k + 1:o + k + 5].tobytes(), "little"))
                allowed[o + k + 1:o + k + 5] = True
        assert c.get("len1", np.uint64).tolist() == exp1 and c.get("stored", np.uint32).tolist() == exps, tag
        assert c.written("len1").all() and c.written("stored").all(), tag + ": the SST arrays for exactly cap slots"
    # ---- (a) the image: bytewise, inside what the call may read
    base, rd, _ = c.mem.touched(d_img)
    lo = d_img - base
    stray = rd.copy()
    stray[lo:lo + n][allowed] = False
    assert not stray.any(), "%s: image of %d bytes read at offset %d" % (tag, n, int(np.nonzero(stray)[0][0]) - lo)
    if table:
        crc_rd = c.reads("crc", 4)
        assert not crc_rd[1:].any(), tag + ": the walk reads crc[0] only"
    c.check(granule_image=True)


# ------------------------------------------------------------------------------------------------- the tables
@pytest.fixture(scope="module")
def tables():
    out = {}
    for name, nblocks, interval in (("0", 0, 1), ("1", 1, 1), ("65", 65, 1), ("65/16", 65, 16), ("300", 300, 1)):
        img, off, ln, meta, index = T.build_table(nblocks, interval, block_len=lambda i: 9 + i % 7, seed=3)
        out[name] = (img, index)
    return out


def damaged(img, index):
    """Two errors in the 65-block table's index: shared = 1 on run 40's first entry, no room for a handle in run 9."""
    ioff, ilen = index
    b = img.copy()
    nr = int.from_bytes(b[ioff + ilen - 4:ioff + ilen].tobytes(), "little")
    ro = ioff + ilen - 4 * (1 + nr)
    restart = lambda r: int.from_bytes(b[ro + 4 * r:ro + 4 * r + 4].tobytes(), "little")
    b[ioff + restart(40)] = 1
    b[ioff + restart(9) + 2] = 0
    return b


@pytest.mark.parametrize("which,skew,cap_delta,spare", [
    ("0", 0, 0, 0), ("0", 4095, 3, 2), ("1", 1, 0, 0), ("1", 15, -1, 300), ("65", 0, 0, 0), ("65", 4095, -1, 3),
    ("65", 1, 3, 200), ("65/16", 15, 0, 0), ("65/16", 4095, 3, 260), ("300", 4095, -1, 0), ("300", 0, 3, 1)])
def test_walk(env, geo, tables, which, skew, cap_delta, spare):
    """kvsep_sst_index_device: `spare` runs of scratch beyond the block's restart count (more workgroups, idle lanes)."""
    img, index = tables[which]
    nblocks = int(which.split("/")[0])
    nr = int.from_bytes(img[index[0] + index[1] - 4:index[0] + index[1]].tobytes(), "little")
    run(env, geo, "sst walk %s skew %d cap%+d runs+%d" % (which, skew, cap_delta, spare), img,
        max(nblocks + cap_delta, 0), nr + spare, skew, False, index)


@pytest.mark.parametrize("case", ["two errors", "over the scratch", "short block", "handle leaves the image",
                                  "handle wraps"])
def test_walk_errors(env, geo, tables, case):
    img, index = tables["65"]
    n = img.size
    if case == "two errors":
        run(env, geo, "sst walk " + case, damaged(img, index), 70, 300, 4095, False, index)
    elif case == "over the scratch":  # the restart count is device data: nothing is written past the scratch
        run(env, geo, "sst walk " + case, img, 70, 64, 1, False, index)
    elif case == "short block":
        run(env, geo, "sst walk " + case, img, 4, 5, 15, False, (index[0], 3))
    elif case == "handle leaves the image":
        run(env, geo, "sst walk " + case, img, 4, 5, 4095, False, (index[0], n - index[0] - 4))
    else:
        run(env, geo, "sst walk " + case, img, 4, 5, 4095, False, (M64 - 2, 10))


@pytest.mark.parametrize("which,skew,cap_delta", [("0", 4095, 2), ("1", 0, 2), ("65", 4095, 2), ("65", 1, 5),
                                                  ("65", 15, 0), ("65/16", 0, 3), ("300", 4095, 2)])
def test_table(env, geo, tables, which, skew, cap_delta):
    """kvsep_sst_table_verify_device without its CRC calls; cap_delta = 2 is exact, below it the slots do not hold
    every block (KVSEP_SST_CAP)."""
    img, index = tables[which]
    nblocks = int(which.split("/")[0])
    run(env, geo, "sst table %s skew %d cap%+d" % (which, skew, cap_delta), img, max(nblocks + cap_delta, 2),
        nblocks + 7, skew, True)


@pytest.mark.parametrize("case", ["wrong magic", "47 bytes", "index leaves the file", "index checksum",
                                  "index compressed", "handles that leave the file"])
def test_table_errors(env, geo, tables, case):
    img, index = tables["65"]
    ioff, ilen = index
    n = img.size
    tag = "sst table " + case
    if case == "wrong magic":
        b = img.copy()
        b[-3] ^= 0x40
        run(env, geo, tag, b, 70, 72, 4095, True)
    elif case == "47 bytes":
        run(env, geo, tag, img[-47:], 5, 8, 4095, True)
    elif case == "index leaves the file":
        b = img.copy()
        b[-48:] = np.frombuffer(T.footer((ioff - 13, 8), (ioff, ilen + 49)), np.uint8)
        run(env, geo, tag, b, 70, 72, 4095, True)
    elif case == "index checksum":
        run(env, geo, tag, img, 70, 72, 4095, True, crc_ok=False)
    elif case == "index compressed":
        b = img.copy()
        b[ioff + ilen:ioff + ilen + 5] = np.frombuffer(T.trailer(img[ioff:ioff + ilen].tobytes(), 1), np.uint8)
        run(env, geo, tag, b, 70, 72, 1, True)
    else:  # emitted handles at off + len + 5 = n + 1 and past 2^64: reported bad, no byte of them addressed
        keys, handles = T.parse_index(img[ioff:ioff + ilen].tobytes())
        handles[5] = (2 ** 64 - 2, 7)
        handles[3] = handles[7] = (n, 0)  # placeholders of the final varint width
        n2 = ioff + len(T.index_block(keys, handles, 1)) + 5 + 48
        handles[3] = (n2 - 4, 0)
        handles[7] = (n2 - 5, 0)  # off + len + 5 = n: usable, its stored word is the image's last four bytes
        blk = T.index_block(keys, handles, 1)
        wild = img[:ioff].tobytes() + blk + T.trailer(blk) + T.footer((ioff - 13, 8), (ioff, len(blk)))
        assert len(wild) == n2
        run(env, geo, tag, wild, 67, 72, 4095, True)


def test_every_kernel_of_the_file_is_run():
    """The kernels of crc32c_sstindex.inc are the ones named here: none is skipped."""
    import re
    src = open(os.path.join(CSRC, "crc32c_sstindex.inc")).read()
    names = set(re.findall(r"\n(sst_[a-z_]+)_kernel\(", src)) | set(re.findall(r"\) (sst_[a-z_]+)_kernel\(", src))
    assert names == {k for k in K if k.startswith("sst_")}, names
