"""The memory envelope of the framing, layout, log and list kernels: the shipped gfx950 assembly reads and writes exactly what
the kernels' header comments promise, and a replay reads no scratch word it did not write.  CPU only.

tests/test_isa_envelope.py does this for the CRC kernels; this file runs, under tools/wave_emu.py, every kernel of

  crc32c_offsets.inc    offsets_tile_sum / tile_scan / write
  crc32c_verdicts.inc   verdict_tile_count / tile_scan / scatter
  crc32c_logwalk.inc    log_count / fill / block / stop / accept / totals
  crc32c_logchain.inc   chain_tile / scan / write / reclen
  crc32c_logframe.inc   logw_layout / fill
  crc32c_concat.inc     crc32c_concat_kernel
  crc32c_pack.inc       crc32c_pack_kernel<PackPlain / PackVlog / PackSst / PackLog>

-- all 23; none is skipped.  The pack kernel's grid depends on a workgroup target the launch code takes from the CU
count; here the target is 4, which pack::team_size turns into its minimum team (the team's arithmetic is the same).

Each call runs as its whole stream-ordered chain in one emulated Memory (count, offsets pass, fill; block, stop, accept,
totals; ...).  The grids and block sizes come from tests/cpp/launch_geometry.cc, a host program over the same pure
headers (concat_run.h, pack_run.h, offsets_run.h, log_run.h, chain_run.h, logw_run.h) the launch code uses; the struct arguments are laid out from
the struct definitions in the .inc files and checked against the size in the kernels' .args metadata
(wave_emu.struct_kernarg).  Per run:

 a. reads: every caller array is a region of exactly its documented element count (an empty or absent one is an
    unmapped address, a null pointer is passed for an absent one), so a read past it is the emulator's "bad address";
    the walked arrays the accept and chains passes read are regions of exactly min(*nrec, cap) elements for the same
    reason; read marks are asserted where a comment makes a read conditional: seg_len only for kept blocks, off[] only
    for a laid record; a segment or block that must not be dereferenced points at 1 << 40.  A log image or pack payload
    sits in a guard region at 0, 1, 15 or 4095 bytes past a 4 KiB boundary with no slack behind it.  The log image is
    read inside [0, n) only -- bytewise, as crc32c_logwalk.inc says, so no granule is allowed; the pack payload inside
    the naturally aligned 16-B granules that hold a byte of a segment of a block that fits its destination;
 b. writes: exactly the documented output elements carry a write mark -- every byte of them, the padding up to cap /
    frag_cap included -- and nothing else but the call's scratch does;
 c. replay soundness: the scratch is filled with 0xA5 and declared scratch (Memory.declare_scratch): no read of a
    scratch byte that this call has not stored;
 d. results: equal to an independent host reference (kvsep.log_walk, log_accept_gaps, log_chains, log_frame_layout,
    vlog_frame_offsets, a serial saturating sum, kvsep.mask, kvsep.combine folded serially, a bytewise gather with
    kvsep.extend_host's CRCs in the frames), never the tests/cpp emulate() models;
 e. cost: the wave-instructions of each case are printed (pytest -s shows them).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kv-separate_amd")
CSRC = os.path.join(PKG, "csrc")
ASM = os.path.join(PKG, "build", "crc32c_device-hip-amdgcn-amd-amdhsa-gfx950.s")
sys.path.insert(0, os.path.join(PKG, "tools"))
sys.path.insert(0, PKG)

from framing_builders import ref_offsets  # noqa: E402  (the serial offsets loop, shared with the forms soak)

M64 = (1 << 64) - 1
SKIP = M64
FAR = 1 << 40  # an address no region of the emulated memory reaches
SKEWS = [0, 1, 15, 4095]
GUARD = 4096

K = {"offsets_tile_sum": "_ZN5kvsep23offsets_tile_sum_kernelENS_11OffsetsArgsE",
     "offsets_tile_scan": "_ZN5kvsep24offsets_tile_scan_kernelEPKyS1_PyS2_m",
     "offsets_write": "_ZN5kvsep20offsets_write_kernelENS_11OffsetsArgsE",
     "verdict_tile_count": "_ZN5kvsep25verdict_tile_count_kernelEPKjS1_mPKyPhPj",
     "verdict_tile_scan": "_ZN5kvsep24verdict_tile_scan_kernelEPKjPyjPKy",
     "verdict_scatter": "_ZN5kvsep22verdict_scatter_kernelEPKjS1_mPKyS3_Pmm",
     "log_count": "_ZN5kvsep16log_count_kernelEPKhmmPy",
     "log_fill": "_ZN5kvsep15log_fill_kernelENS_11LogWalkArgsE",
     "log_block": "_ZN5kvsep16log_block_kernelENS_13LogAcceptArgsE",
     "log_stop": "_ZN5kvsep15log_stop_kernelEPKymPy",
     "log_accept": "_ZN5kvsep17log_accept_kernelENS_13LogAcceptArgsE",
     "log_totals": "_ZN5kvsep17log_totals_kernelEPKyS1_mPmS2_",
     "chain_tile": "_ZN5kvsep17chain_tile_kernelENS_9ChainArgsE",
     "chain_scan": "_ZN5kvsep17chain_scan_kernelEPKyPyS2_m",
     "chain_write": "_ZN5kvsep18chain_write_kernelENS_9ChainArgsE",
     "chain_reclen": "_ZN5kvsep19chain_reclen_kernelEPKyPmm",
     "logw_layout": "_ZN5kvsep18logw_layout_kernelENS_8LogwArgsE",
     "logw_fill": "_ZN5kvsep16logw_fill_kernelENS_8LogwArgsE",
     "concat": "_ZN5kvsep20crc32c_concat_kernelEPKjPKmS3_S1_PjmmPKNS_9DevTablesE",
     "pack_plain": "_ZN5kvsep18crc32c_pack_kernelINS_9PackPlainEEEvNS_8PackArgsE",
     "pack_vlog": "_ZN5kvsep18crc32c_pack_kernelINS_8PackVlogEEEvNS_8PackArgsE",
     "pack_sst": "_ZN5kvsep18crc32c_pack_kernelINS_7PackSstEEEvNS_8PackArgsE",
     "pack_log": "_ZN5kvsep18crc32c_pack_kernelINS_7PackLogEEEvNS_8PackArgsE"}
STRUCTS = {"OffsetsArgs": "crc32c_offsets.inc", "LogWalkArgs": "crc32c_logwalk.inc", "LogAcceptArgs": "crc32c_logwalk.inc",
           "ChainArgs": "crc32c_logchain.inc", "LogwArgs": "crc32c_logframe.inc"}


class Env:
    def __init__(self, tmp):
        import wave_emu
        self.E = wave_emu
        self.exe = os.path.join(tmp, "launch_geometry")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                               os.path.join(ROOT, "tests", "cpp", "launch_geometry.cc"), "-o", self.exe])
        self.const = {k: int(v) for k, v in (ln.split() for ln in self._ask("constants"))}
        self.cost = {}

    def _ask(self, *args):
        return subprocess.check_output([self.exe] + [str(a) for a in args], text=True).splitlines()

    def tables(self):
        """The DevTables image (crc32c_concat_kernel reads its x2n), built once."""
        if not hasattr(self, "_tables"):
            self._tables = self.E.dev_tables()
        return self._tables

    def const_threads(self, family):
        return int(self._ask(family, 1, 4)[0].split()[2])

    def scratch(self, family, n):
        """{"words": the words an array sized for n holds, slice: its word offset} from the pure header of `family`."""
        return {k: int(v) for k, v in (ln.split() for ln in self._ask("scratch", family, n))}

    def tile_words(self, c, count):
        """The offsets pass's tile array for `count` blocks and its slices, as OffsetsArgs fields."""
        w = self.scratch("offsets", count)
        tile = c.scratch("tile", 8 * w.pop("words"))
        return {k: tile + 8 * at for k, at in w.items()}

    def geometry(self, *args):
        """[(kernel, grid, threads)] of a call, in stream order, from tests/cpp/launch_geometry.cc."""
        return [(k, int(g), int(t)) for k, g, t in (ln.split() for ln in self._ask(*args))]


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-s", "-C", PKG, "asm"], stdout=subprocess.DEVNULL)
    return Env(str(tmp_path_factory.mktemp("geometry")))


class Call:
    """One call's device image: caller arrays of exactly their size, outputs, scratch; then the checks."""

    def __init__(self, env, tag):
        self.env, self.E, self.tag = env, env.E, tag
        self.mem = env.E.Memory(track=True)
        self.kind = {}   # region base -> ("in" | "out" | "scratch", name)
        self.addr = {}   # name -> address (FAR-based for an empty array)
        self.size = {}
        self.steps = 0
        self.nowhere = FAR

    def _place(self, name, nbytes, kind, data=None):
        if nbytes == 0:  # an empty array: any access is a bad address
            self.nowhere += 1 << 20
            self.addr[name], self.size[name] = self.nowhere, 0
            return self.nowhere
        base = self.mem.alloc(nbytes, data=data)
        self.kind[base] = (kind, name)
        self.addr[name], self.size[name] = base, nbytes
        return base

    def input(self, name, arr):
        arr = np.ascontiguousarray(arr)
        return self._place(name, arr.nbytes, "in", arr if arr.nbytes else None)

    def output(self, name, nbytes):
        return self._place(name, nbytes, "out", np.full(nbytes, 0xCC, np.uint8) if nbytes else None)

    def scratch(self, name, nbytes):
        base = self._place(name, nbytes, "scratch", np.full(nbytes, 0xA5, np.uint8) if nbytes else None)
        if nbytes:
            self.mem.declare_scratch(base)
        return base

    def image(self, data, skew):
        """The log image in a guard region: its first byte `skew` past a 4 KiB boundary, GUARD tracked bytes before
        and after it and no slack."""
        data = np.ascontiguousarray(data, np.uint8)
        region = self.mem.alloc(GUARD + data.size + GUARD, align=4096, data=data if data.size else None,
                                phase=(skew - GUARD) % 4096, at=GUARD)
        self.kind[region] = ("image", "image")
        self.img = (region, region + GUARD, data.size)
        assert (region + GUARD) % 4096 == skew
        return region + GUARD

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

    def get(self, name, dtype):
        return self.mem.view(self.addr[name], self.size[name]).view(dtype).copy() if self.size[name] else \
            np.zeros(0, dtype)

    def reads(self, name, itemsize):
        """Per element of array `name`: was any of its bytes read."""
        if not self.size[name]:
            return np.zeros(0, bool)
        return self.mem.touched(self.addr[name])[1].reshape(-1, itemsize).any(axis=1)

    def check(self, partial_out=(), granule_image=False):
        """(a) for the image, (b) and (c) for everything; partial_out: outputs whose written bytes the caller checks."""
        mem = self.mem
        for base, (kind, name) in self.kind.items():
            _, rd, wr = mem.touched(base)
            if kind == "in":
                assert not wr.any(), "%s: input %s written at byte %d" % (self.tag, name, np.nonzero(wr)[0][0])
            elif kind == "out" and name not in partial_out:
                assert wr.all(), "%s: output %s: bytes never written: %s ..." % (self.tag, name, np.nonzero(~wr)[0][:8])
            elif kind == "image":
                assert not wr.any(), "%s: the image was written" % self.tag
                _, pay, n = self.img
                lo = pay - base
                out = rd.copy()
                out[lo:lo + n] = False
                assert granule_image or not out.any(), "%s: image of %d bytes read at offset %d" % (
                    self.tag, n, int(np.nonzero(out)[0][0]) - lo)  # (granule_image: the caller checks the granules)
        assert not mem.uninit, "%s: scratch read before this call wrote it: %s" % (
            self.tag, ["0x%x (+%d) at line %d" % u for u in mem.uninit[:4]])
        self.env.cost[self.tag] = self.steps
        print("%-60s %9d wave-instructions" % (self.tag, self.steps))


# ===================================================================================================== offsets
def run_offsets(env, tag, seg_len, first, keep, before, head, tail, start, max_size, count, nkept_word=True):
    c = Call(env, tag)
    nseg = len(seg_len)
    geo = env.geometry("offsets", count)
    nt = geo[0][1]
    v = dict(seg_len=c.input("seg_len", np.asarray(seg_len, np.uint64)), head=head, tail=tail, start=start,
             max_size=max_size, count=count, nseg=nseg, dst_off=c.output("dst_off", 8 * count), end=c.output("end", 8))
    if first is not None:
        v["first"] = c.input("first", np.asarray(first, np.uint64))
    if keep is not None:
        v["keep"] = c.input("keep", np.asarray(keep, np.uint8))
    if before is not None:
        v["keep_before"] = c.input("keep_before", np.array([before], np.uint64))
    if nkept_word:
        v["nkept"] = c.output("nkept", 8)
    if nt:  # the launch code's carve-up of the pass's two allocations
        v["ext"] = c.scratch("ext", 8 * count)
        v.update(env.tile_words(c, count))
    args = c.sargs("offsets_tile_sum", "OffsetsArgs", v)
    for kernel, grid, threads in geo:
        if not grid:
            continue
        if kernel == "offsets_tile_scan_kernel":
            c.launch("offsets_tile_scan", grid, threads, c.pargs("offsets_tile_scan", [
                v["tile_sum"], v["tile_kept"], v["tile_base"], v["grand"], nt]))
        else:
            c.launch(kernel[:-7], grid, threads, args)
    exp, end, nk, kept_segs = ref_offsets(seg_len, first, keep, before, head, tail, start, max_size, count)
    got = c.get("dst_off", np.uint64)
    assert np.array_equal(got, exp), "%s: dst_off differs at %s" % (tag, np.nonzero(got != exp)[0][:8])
    assert int(c.get("end", np.uint64)[0]) == end, tag
    if nkept_word:
        assert int(c.get("nkept", np.uint64)[0]) == nk, tag
    rd = np.nonzero(c.reads("seg_len", 8))[0]
    assert set(rd.tolist()) == kept_segs, "%s: seg_len read at %s, outside the kept blocks' runs" % (
        tag, sorted(set(rd.tolist()) - kept_segs)[:8])
    if first is not None:  # "first for count + 1 elements": read for dropped blocks too, their runs are not
        assert c.reads("first", 8).all() or count == 0
    c.check()
    return c


def offsets_counts(env):
    t = env.const["offsets_kTile"]
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("ci", range(9))
def test_offsets_plain_and_masked(env, ci):
    """Every count, block i = segment i: no rule, then ok[] bytes with dropped blocks at the row and tile edges."""
    count = offsets_counts(env)[ci]
    rng = np.random.default_rng(100 + ci)
    seg = rng.integers(0, 5000, count).astype(np.uint64)
    run_offsets(env, "offsets count %d plain" % count, seg, None, None, None, 8, 0, 12345, (1 << 32) - 1, count)
    if count:
        from kvsep import vlog_frame_offsets
        rec_off, end = vlog_frame_offsets(seg, 12345)
        exp = ref_offsets(seg, None, None, None, 8, 0, 12345, (1 << 32) - 1, count)
        assert np.array_equal(rec_off, exp[0]) and end == exp[1]  # the serial reference agrees with the host form
        keep = rng.integers(0, 2, count).astype(np.uint8)
        for e in (0, 62, 63, 64, 65, 1023, 1024, count - 1):
            if e < count:
                keep[e] = e % 2
        run_offsets(env, "offsets count %d keep[]" % count, seg, None, keep, None, 8, 4, 0, M64, count,
                    nkept_word=False)


@pytest.mark.parametrize("count", [65, "tile+1"])
@pytest.mark.parametrize("rule", ["none", "keep", "before0", "beforemid", "beforecount", "beforepast"])
def test_offsets_runs(env, count, rule):
    """first[] runs (empty, short, and longer than a wave's 64 lanes so the wave-wide sum runs), every keep rule."""
    count = env.const["offsets_kTile"] + 1 if count == "tile+1" else count
    rng = np.random.default_rng(7 * count + len(rule))
    runs = rng.integers(0, 4, count)
    runs[[1, count // 2, count - 1]] = [70, 129, 64 + 17]  # long runs: first rows, middle, the very last block
    runs[0] = 0
    first = np.zeros(count + 1, np.uint64)
    first[1:] = np.cumsum(runs)
    nseg = int(first[-1])
    seg = rng.integers(0, 3000, nseg).astype(np.uint64)
    keep = before = None
    if rule == "keep":
        keep = rng.integers(0, 2, count).astype(np.uint8)
        keep[[1, count - 1]] = [0, 1]  # one long run dropped (never read), one kept
    elif rule != "none":
        before = {"before0": 0, "beforemid": count // 2, "beforecount": count, "beforepast": count + 5}[rule]
    run_offsets(env, "offsets runs count %d %s" % (count, rule), seg, first, keep, before, 3, 5, 1 << 33, M64, count)


def test_offsets_saturating(env):
    """One extent of 2^64 - 1: that block and every kept block after it get kSkip, *end saturates."""
    count = 130
    seg = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(1000)
    seg[70] = np.uint64(M64)
    keep = np.ones(count, np.uint8)
    keep[[5, 100]] = 0
    c = run_offsets(env, "offsets saturating", seg, None, keep, None, 8, 0, 0, M64, count)
    got = c.get("dst_off", np.uint64)
    assert (got[70:] == np.uint64(SKIP)).all() and got[69] != np.uint64(SKIP)
    # and a length over max_size counts as saturated
    seg[70] = np.uint64(1 << 32)
    run_offsets(env, "offsets over max_size", seg, None, None, None, 8, 0, 0, (1 << 32) - 1, count)


# ===================================================================================================== verdicts
@pytest.mark.parametrize("count", [1, 255, 256, 257, "tile+1"])
@pytest.mark.parametrize("cap", ["zero", "short", "exact"])
def test_verdicts(env, count, cap):
    from kvsep import mask
    count = env.const["list_kTile"] + 1 if count == "tile+1" else count
    rng = np.random.default_rng(count)
    out = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    stored = np.array([mask(int(x)) for x in out], np.uint32)
    bad = np.unique(np.concatenate([[0, count - 1], rng.integers(0, count, 9)]))
    bad = bad[bad % 5 != 3] if count > 1 else bad
    stored[bad] ^= 0x40
    nbad = bad.size
    bad_cap = {"zero": 0, "short": max(nbad - 1, 0), "exact": nbad}[cap]
    tag = "verdicts count %d bad_cap %d of %d" % (count, bad_cap, nbad)
    c = Call(env, tag)
    geo = env.geometry("verdicts", count)
    nt = geo[0][1]
    d_out, d_st = c.input("out", out), c.input("stored", stored)
    d_nbad = c.input("nbad", np.array([nbad], np.uint64))
    d_ok = c.output("ok", count)
    d_idx = c.output("bad_idx", 8 * bad_cap)
    d_cnt = c.scratch("tile_cnt", 4 * nt) if bad_cap else 0
    d_base = c.scratch("tile_base", 8 * nt) if bad_cap else 0
    c.launch("verdict_tile_count", geo[0][1], geo[0][2], c.pargs("verdict_tile_count", [
        d_out, d_st, count, d_nbad, d_ok, d_cnt]))
    if bad_cap:  # launch_list: no list wanted, no scan and no scatter
        c.launch("verdict_tile_scan", geo[1][1], geo[1][2], c.pargs("verdict_tile_scan", [d_cnt, d_base, nt, d_nbad]))
        c.launch("verdict_scatter", geo[2][1], geo[2][2], c.pargs("verdict_scatter", [
            d_out, d_st, count, d_nbad, d_base, d_idx, bad_cap]))
    ok = np.ones(count, np.uint8)
    ok[bad] = 0
    assert np.array_equal(c.get("ok", np.uint8), ok), tag
    assert np.array_equal(c.get("bad_idx", np.uint64), bad[:bad_cap].astype(np.uint64)), tag
    c.check()


# ===================================================================================================== chains
FULL, FIRST, MIDDLE, LAST = 1, 2, 3, 4


def chain_records(count, rng):
    ty = rng.choice([FULL, FIRST, MIDDLE, LAST, 5, 0], count, p=[.25, .2, .25, .2, .05, .05]).astype(np.uint8)
    acc = (rng.random(count) < 0.9).astype(np.uint8)
    gap = (rng.random(count) < 0.08).astype(np.uint8)
    for a in (61, 1021):  # a FIRST ... LAST chain across lane 63 / 64 and across record 1023 / 1024
        if a + 5 <= count:
            ty[a:a + 5] = [FIRST, MIDDLE, MIDDLE, MIDDLE, LAST]
            acc[a:a + 5] = 1
            gap[a:a + 5] = 0
    return ty, acc, gap


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, "tile", "tile+1"])
@pytest.mark.parametrize("form", ["bare", "gap", "frags"])
def test_chains(env, count, form):
    from kvsep import log_chains
    t = env.const["chain_kTile"]
    count = {"tile": t, "tile+1": t + 1}.get(count, count)
    rng = np.random.default_rng(count + 31)
    ty, acc, gap = chain_records(count, rng)
    # cap: the record count; three more (padding); one fewer than *nrec says (the arrays cut by cap)
    cap, nrec = {"bare": (count, count), "gap": (count + 3, count), "frags": (count, count + 1)}[form]
    if form == "bare":
        gap = None
    tag = "chains count %d %s" % (count, form)
    c = Call(env, tag)
    geo = env.geometry("chains", cap)
    nt = geo[0][1]
    v = dict(type=c.input("type", ty), accept=c.input("accept", acc), nrec=c.input("nrec", np.array([nrec], np.uint64)),
             cap=cap, ntiles=nt, first=c.output("first", 8 * (cap + 1)), whole=c.output("whole", cap),
             nchain=c.output("nchain", 8))
    if gap is not None:
        v["gap"] = c.input("gap", gap)
    off = (np.arange(count, dtype=np.uint64) * np.uint64(40) + np.uint64(6))
    ln = rng.integers(1, 30, count).astype(np.uint64)
    if form == "frags":
        v.update(off=c.input("off", off), len=c.input("len", ln), frag_off=c.output("frag_off", 8 * cap),
                 frag_len=c.output("frag_len", 8 * cap), nwhole=c.output("nwhole", 8))
    if nt:
        w = env.scratch("chains", cap)
        sc = c.scratch("chain", 8 * w.pop("words"))
        v.update({k: sc + 8 * at for k, at in w.items()})
    args = c.sargs("chain_tile", "ChainArgs", v)
    c.launch("chain_tile", geo[0][1], geo[0][2], args)
    if nt:
        c.launch("chain_scan", geo[1][1], geo[1][2], c.pargs("chain_scan", [v["sum"], v["in"], v["grand"], nt]))
    c.launch("chain_write", geo[2][1], geo[2][2], args)
    first, whole, nchain, nwhole = log_chains(ty, acc, gap)
    exp_first = np.full(cap + 1, count, np.uint64)
    exp_first[:nchain] = first[:nchain]
    exp_whole = np.zeros(cap, np.uint8)
    exp_whole[:nchain] = whole[:nchain]
    assert int(c.get("nchain", np.uint64)[0]) == nchain, tag
    assert np.array_equal(c.get("first", np.uint64), exp_first), tag
    assert np.array_equal(c.get("whole", np.uint8), exp_whole), tag
    if form == "frags":
        assert int(c.get("nwhole", np.uint64)[0]) == nwhole, tag
        fo, fl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        fo[:count], fl[:count] = off + np.uint64(1), ln - np.uint64(1)
        assert np.array_equal(c.get("frag_off", np.uint64), fo) and np.array_equal(c.get("frag_len", np.uint64), fl), tag
    c.check()


def test_chain_reclen(env):
    """rec_len[j] = ext[j] for j < cap: ext and rec_len exactly cap long, cap one past a workgroup."""
    cap = env.geometry("chains", 1)[3][2] + 1
    c = Call(env, "chain_reclen cap %d" % cap)
    ext = np.arange(cap, dtype=np.uint64) * np.uint64(977) + np.uint64(1 << 40)
    kernel, grid, threads = env.geometry("chains", cap)[3]
    c.launch("chain_reclen", grid, threads, c.pargs("chain_reclen", [c.input("ext", ext), c.output("rec_len", 8 * cap),
                                                                     cap]))
    assert np.array_equal(c.get("rec_len", np.uint64), ext)
    assert c.reads("ext", 8).all()
    c.check()


# ===================================================================================================== log frame
SEEDS = {FULL: 0x11111111, FIRST: 0x22222222, MIDDLE: 0x33333333, LAST: 0x44444444}


def ref_fragments(env, ln, rec_at, b0):
    """Every fragment of the laid records by log::Writer::AddRecord's loop (db/log_writer.cc:35-82), and the pad
    zeros (relative to the first appended byte) in front of each record's first header."""
    B, H = env.const["logw_kBlock"], 7
    frags, pads, prev_end = [], {}, 0
    for i, at in enumerate(rec_at):
        if at == SKIP:
            continue
        if at > prev_end:
            pads[i] = (prev_end, at)
        pos, left, begin, k = at + b0, int(ln[i]), 0, 0
        while True:
            room = B - pos % B - H
            take = min(left, room)
            last = take == left
            ftype = (FULL if last else FIRST) if k == 0 else (LAST if last else MIDDLE)
            frags.append((i, begin, take, pos - b0, ftype))
            pos += H + take
            begin += take
            left -= take
            k += 1
            if last:
                break
        prev_end = pos - b0
    return frags, pads


def run_logw(env, tag, ln, keep, dest_length, extra_cap, short_dst=0):
    from kvsep import log_frame_layout
    ln = np.asarray(ln, np.uint64)
    count = ln.size
    rec_at, frag_first, nfrag, written = log_frame_layout(ln, keep, dest_length)
    b0 = dest_length % env.const["logw_kBlock"]
    frag_cap, dst_bytes = nfrag + extra_cap, written - short_dst
    c = Call(env, tag)
    geo = env.geometry("logw", count, frag_cap)
    off = np.arange(count, dtype=np.uint64) * np.uint64(1 << 20) + np.uint64(77)
    v = dict(len=c.input("len", ln), off=c.input("off", off), count=count, b0=b0, dst=c.output("dst", dst_bytes),
             dst_bytes=dst_bytes, rec_at=c.output("rec_at", 8 * count), frag_first=c.output("frag_first", 8 * (count + 1)),
             frag_off=c.output("frag_off", 8 * frag_cap), frag_len=c.output("frag_len", 8 * frag_cap),
             frag_at=c.output("frag_at", 8 * frag_cap), frag_type=c.output("frag_type", frag_cap), frag_cap=frag_cap,
             nfrag=c.output("nfrag", 8), written=c.output("written", 8), rec=c.scratch("rec", 4 * count),
             seed=c.scratch("seed", 4 * frag_cap), s1=SEEDS[FULL], s2=SEEDS[FIRST], s3=SEEDS[MIDDLE], s4=SEEDS[LAST])
    if keep is not None:
        v["keep"] = c.input("keep", np.asarray(keep, np.uint8))
    args = c.sargs("logw_layout", "LogwArgs", v)
    for kernel, grid, threads in geo:
        c.launch(kernel[:-7], grid, threads, args)
    assert int(c.get("nfrag", np.uint64)[0]) == nfrag and int(c.get("written", np.uint64)[0]) == written, tag
    assert np.array_equal(c.get("rec_at", np.uint64), rec_at), tag
    assert np.array_equal(c.get("frag_first", np.uint64), frag_first), tag
    frags, pads = ref_fragments(env, ln, [int(x) for x in rec_at], b0)
    assert len(frags) == nfrag
    e_off, e_len, e_at = np.zeros(frag_cap, np.uint64), np.zeros(frag_cap, np.uint64), np.full(frag_cap, SKIP, np.uint64)
    e_type, e_seed = np.zeros(frag_cap, np.uint8), np.zeros(frag_cap, np.uint32)
    laid = set()
    for f, (i, begin, take, at, ftype) in enumerate(frags[:frag_cap]):
        e_off[f], e_len[f], e_at[f], e_type[f], e_seed[f] = int(off[i]) + begin, take, at, ftype, SEEDS[ftype]
        laid.add(i)
    for name, exp, dt in (("frag_off", e_off, np.uint64), ("frag_len", e_len, np.uint64), ("frag_at", e_at, np.uint64),
                          ("frag_type", e_type, np.uint8), ("seed", e_seed, np.uint32)):
        got = c.get(name, dt)
        assert np.array_equal(got, exp), "%s: %s differs at %s" % (tag, name, np.nonzero(got != exp)[0][:8])
    # off[] only for a laid record
    rd = set(np.nonzero(c.reads("off", 8))[0].tolist())
    assert rd <= laid, "%s: off[] read for records %s that own no stored fragment" % (tag, sorted(rd - laid)[:8])
    # dst: exactly the pad zeros of the records whose first fragment is stored, inside [0, dst_bytes)
    want = np.zeros(dst_bytes, bool)
    for i, (lo, hi) in pads.items():
        if int(frag_first[i]) < frag_cap and hi <= dst_bytes:
            want[lo:hi] = True
    if dst_bytes:
        _, _, wr = c.mem.touched(c.addr["dst"])
        assert np.array_equal(wr, want), "%s: dst written at %s, pad zeros expected at %s" % (
            tag, np.nonzero(wr)[0][:8], np.nonzero(want)[0][:8])
        assert (c.get("dst", np.uint8)[want] == 0).all()
    # the scratch words: rec for exactly count, seed for exactly frag_cap
    for name in ("rec", "seed"):
        if c.size[name]:
            assert c.mem.touched(c.addr[name])[2].all(), "%s: %s not written in full" % (tag, name)
    c.check(partial_out=("dst",))
    return c


def logw_counts(env):
    a = env.const["logw_kAhead"] * env.const["logw_kWaveLanes"]
    return [0, 1, 63, 64, 65, a - 1, a, a + 1]


@pytest.mark.parametrize("ci", range(8))
@pytest.mark.parametrize("residue", [0, 32761, 32762])
def test_log_frame(env, ci, residue):
    """Every count at every dest_length residue: keep null with frag_cap = *nfrag, then dropped records at the row
    edges with three slots of padding.  Lengths up to 3,000, so a row of 64 crosses several 32 KiB blocks."""
    count = logw_counts(env)[ci]
    rng = np.random.default_rng(1000 * ci + residue)
    ln = rng.integers(0, 3000, count).astype(np.uint64)
    if count > 2:
        ln[count // 2] = 0
    dest = 5 * 32768 + residue
    run_logw(env, "logw count %d residue %d keep null" % (count, residue), ln, None, dest, 0)
    if count:
        keep = (rng.random(count) < 0.8).astype(np.uint8)
        for e in (0, 62, 63, 64, 65, 127, 128, count - 1):
            if e < count:
                keep[e] = (e + ci) % 2
        run_logw(env, "logw count %d residue %d keep[]" % (count, residue), ln, keep, dest, 3)


def test_log_frame_long_record_and_block_ends(env):
    """A record longer than a block (FIRST, MIDDLE, LAST), records that leave 0 .. 7 bytes in their block (the lazy pad
    of the next one), and a short dst: the pad zeros past dst_bytes are not written."""
    B = env.const["logw_kBlock"]
    ln = [100, 3 * B + 5, 10]
    for left in range(8):  # after each: a record that ends `left` bytes before its block's end, then a small one
        ln += [None, 3]
    ln = list(ln)
    pos = 0
    out = []
    for x in ln:
        if x is None:
            left = (len(out) - 3) // 2
            room = B - pos % B
            x = room - 7 - left if room - 7 - left >= 0 else room + B - 14 - left  # (a block of its own when too tight)
        # AddRecord's position after this record, for sizing the next filler (checked against the reference below)
        rem = x
        if B - pos % B < 7:
            pos += B - pos % B
        while True:
            take = min(rem, B - pos % B - 7)
            pos += 7 + take
            rem -= take
            if rem == 0:
                break
        out.append(x)
    c = run_logw(env, "logw long record, block ends", out, None, 0, 3)
    assert (c.get("frag_type", np.uint8)[1:5] == [FIRST, MIDDLE, MIDDLE, LAST]).all()
    run_logw(env, "logw short dst", out, None, 0, 0, short_dst=B)


# ===================================================================================================== log read
def log_image(rng, env):
    """Four blocks: the first three end in 0, 1 and 6 trailer bytes; the last is ten zero-length records, a chain, a
    type-5 record and a header whose length runs past the end."""
    B = env.const["log_kBlock"]
    img = bytearray()

    def rec(t, n):
        img.extend(rng.integers(0, 256, 4, dtype=np.uint8).tobytes() + bytes([n & 255, n >> 8, t]) +
                   rng.integers(0, 256, n, dtype=np.uint8).tobytes())

    for trailer in (0, 1, 6):
        end = (len(img) // B + 1) * B - trailer
        while end - len(img) > 4000:
            rec(int(rng.choice([FULL, FIRST, MIDDLE, LAST])), int(rng.integers(0, 3000)))
        rec(FULL, (end - len(img) - 14) // 2)
        rec(LAST, end - len(img) - 7)
        img.extend(bytes(trailer))
    for _ in range(10):
        rec(FULL, 0)
    for t in (FIRST, MIDDLE, LAST, 5, FULL):
        rec(t, 33)
    img.extend(bytes([1, 2, 3, 4, 100, 0, FULL]) + bytes(20))  # length 100, 20 bytes left
    return np.frombuffer(bytes(img), np.uint8).copy()


def run_log(env, tag, img, cap_delta, skew):
    """kvsep_log_walk_device's chain (count, the offsets pass over the counts, fill), then kvsep_log_accept_device's
    (block, stop, accept, totals) on the walk's outputs, the scratch refilled in between: neither call may lean on the
    other's words."""
    from kvsep import log_accept_gaps, log_walk
    n = img.size
    off, ln, st, ty = log_walk(img)
    nrec = off.size
    cap = max(nrec + cap_delta, 0)
    held = min(nrec, cap)
    c = Call(env, tag)
    geo = dict((k, (g, t)) for k, g, t in env.geometry("log", n, cap))
    nb = -(-n // env.const["log_kBlock"])  # the image's 32 KiB blocks
    d_img = c.image(img, skew)
    lw = env.scratch("log", nb)
    words = lw.pop("words")
    d_log = c.scratch("log", 8 * words)
    nt = geo["offsets_tile_sum_kernel"][0]
    d_nrec = c.output("nrec", 8)
    wv = dict(img=d_img, n=n, nblocks=nb, off=c.output("off", 8 * cap), len=c.output("len", 8 * cap),
              stored=c.output("stored", 4 * cap), type=c.output("type", cap), cap=cap, nrec=d_nrec,
              cnt=d_log + 8 * lw["cnt"], base=d_log + 8 * lw["base"])
    c.launch("log_count", *geo["log_count_kernel"], c.pargs("log_count", [d_img, n, nb, wv["cnt"]]))
    ov = dict(seg_len=wv["cnt"], max_size=M64, count=nb, nseg=nb, dst_off=wv["base"], end=d_nrec)
    if nt:
        ov["ext"] = c.scratch("ext", 8 * nb)
        ov.update(env.tile_words(c, nb))
    oargs = c.sargs("offsets_tile_sum", "OffsetsArgs", ov)
    c.launch("offsets_tile_sum", *geo["offsets_tile_sum_kernel"], oargs)
    if nt:
        c.launch("offsets_tile_scan", *geo["offsets_tile_scan_kernel"], c.pargs("offsets_tile_scan", [
            ov["tile_sum"], ov["tile_kept"], ov["tile_base"], ov["grand"], nt]))
    c.launch("offsets_write", *geo["offsets_write_kernel"], oargs)
    c.launch("log_fill", *geo["log_fill_kernel"], c.sargs("log_fill", "LogWalkArgs", wv))
    assert int(c.get("nrec", np.uint64)[0]) == nrec, "%s: *nrec %d, the host walk finds %d" % (
        tag, int(c.get("nrec", np.uint64)[0]), nrec)
    for name, ref, dt in (("off", off, np.uint64), ("len", ln, np.uint64), ("stored", st, np.uint32),
                          ("type", ty, np.uint8)):
        exp = np.zeros(cap, dt)
        exp[:held] = ref[:held]
        got = c.get(name, dt)
        assert np.array_equal(got, exp), "%s: %s differs at %s" % (tag, name, np.nonzero(got != exp)[0][:8])
    c.check()
    walk_steps = c.steps

    # ---- the accept pass: its inputs are arrays of exactly `held` elements
    rng = np.random.default_rng(n + cap)
    ok = (rng.random(held) < 0.9).astype(np.uint8)
    a = Call(env, tag + " accept")
    d_img = a.image(img, skew)
    d_log = a.scratch("log", 8 * words)
    av = dict(img=d_img, n=n, nblocks=nb, off=a.input("off", off[:held]), len=a.input("len", ln[:held]),
              type=a.input("type", ty[:held]), ok=a.input("ok", ok), nrec=a.input("nrec", np.array([nrec], np.uint64)),
              cap=cap, accept=a.output("accept", cap), gap=a.output("gap", cap), dropped=a.output("dropped", 8),
              bad_length=a.output("bad_length", 8),
              **{k: d_log + 8 * lw[k] for k in ("stop", "first", "state", "cand", "drop", "badlen")})
    aargs = a.sargs("log_block", "LogAcceptArgs", av)
    a.launch("log_block", *geo["log_block_kernel"], aargs)
    a.launch("log_stop", *geo["log_stop_kernel"], a.pargs("log_stop", [av["cand"], nb, av["stop"]]))
    a.launch("log_accept", *geo["log_accept_kernel"], aargs)
    a.launch("log_totals", *geo["log_totals_kernel"], a.pargs("log_totals", [
        av["drop"], av["badlen"], nb, av["dropped"], av["bad_length"]]))
    r_acc, r_gap, r_drop, r_bad = log_accept_gaps(img, ok)
    for name, ref in (("accept", r_acc), ("gap", r_gap)):
        exp = np.zeros(cap, np.uint8)
        exp[:held] = ref[:held]
        got = a.get(name, np.uint8)
        assert np.array_equal(got, exp), "%s: %s differs at %s" % (tag, name, np.nonzero(got != exp)[0][:8])
    if held == nrec:  # the byte counts of the whole image: the host form sees only `held` records
        assert (int(a.get("dropped", np.uint64)[0]), int(a.get("bad_length", np.uint64)[0])) == (r_drop, r_bad), tag
    a.steps += walk_steps
    a.check()


@pytest.fixture(scope="module")
def images(env):
    B = env.const["log_kBlock"]
    img = log_image(np.random.default_rng(5), env)
    assert img.size > 3 * B
    cut = img[:2 * B + 27].copy()
    cut[2 * B:2 * B + 7] = [9, 9, 9, 9, 200, 0, FULL]  # two blocks and a header whose 200 bytes run past the end
    one = np.array([1, 2, 3, 4, 0, 0, FULL], np.uint8)
    return {"0": img[:0], "6": img[:6], "7": one, "B-1": img[:B - 1], "B": img[:B], "B+6": img[:B + 6], "2B+header": cut,
            "whole": img}


@pytest.mark.parametrize("which,skew", [("0", 0), ("6", 4095), ("7", 1), ("7", 4095), ("B-1", 15), ("B", 4095),
                                        ("B+6", 1), ("2B+header", 4095), ("whole", 0), ("whole", 1), ("whole", 15),
                                        ("whole", 4095)])
@pytest.mark.parametrize("cap_delta", [0, -1, 3])
def test_log_read(env, images, which, skew, cap_delta):
    run_log(env, "log image %s skew %d cap%+d" % (which, skew, cap_delta), images[which], cap_delta, skew)


# ===================================================================================================== concat
def run_concat(env, tag, runs, with_init, rng, big_lengths=True):
    """Block i is a run of runs[i] segments; seg_crc / seg_len are exactly nseg long, first count + 1, init / out count.
    The reference folds kvsep.combine serially over each run."""
    from kvsep import combine
    count = len(runs)
    first = np.zeros(count + 1, np.uint64)
    first[1:] = np.cumsum(runs)
    nseg = int(first[-1])
    seg_crc = rng.integers(0, 1 << 32, nseg, dtype=np.uint64).astype(np.uint32)
    seg_len = rng.integers(0, 1 << 20, nseg).astype(np.uint64)
    for i in range(count):  # zero-length segments at either end of every run of three or more
        if runs[i] >= 3:
            seg_len[int(first[i])] = seg_len[int(first[i + 1]) - 1] = 0
    if big_lengths and nseg > 8:  # lengths whose 8 n leaves 64 bits: concat_xpow8's top three bits
        seg_len[[1, nseg // 2, nseg - 2]] = [np.uint64(M64), np.uint64(1 << 61), np.uint64((1 << 63) + 12345)]
    init = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32) if with_init else None
    c = Call(env, tag)
    (kernel, grid, threads), = env.geometry("concat", count)
    tabs = c.input("tabs", np.frombuffer(env.tables(), np.uint8))
    args = c.pargs("concat", [c.input("seg_crc", seg_crc), c.input("seg_len", seg_len), c.input("first", first),
                              c.input("init", init) if with_init else 0, c.output("out", 4 * count), count, nseg, tabs])
    c.launch("concat", grid, threads, args)
    exp = np.zeros(count, np.uint32)
    for i in range(count):
        acc = int(init[i]) if with_init else 0
        for j in range(int(first[i]), int(first[i + 1])):
            acc = combine(acc, int(seg_crc[j]), int(seg_len[j]))
        exp[i] = acc
    got = c.get("out", np.uint32)
    assert np.array_equal(got, exp), "%s: out differs at %s" % (tag, np.nonzero(got != exp)[0][:8])
    for name, size in (("seg_crc", 4), ("seg_len", 8), ("first", 8)):
        assert c.reads(name, size).all(), "%s: %s not read in full" % (tag, name)
    c.check()


@pytest.mark.parametrize("with_init", [False, True])
def test_concat(env, with_init):
    """Blocks of 0, 1, 2 and kPerWg + 1 segments (the last a wavefront's long run), at both ends of the batch and at
    the edges of a wavefront's 16 blocks; kPerWg + 1 blocks, so a second workgroup runs with one block; then a run of
    more than one pass (kPassSegs + 3 segments) next to the short / long threshold."""
    per, short, pas = env.const["concat_kPerWg"], env.const["concat_kShortMax"], env.const["concat_kPassSegs"]
    rng = np.random.default_rng(11 + with_init)
    runs = [int(x) for x in rng.choice([0, 1, 2], per + 1)]
    runs[0], runs[1], runs[15], runs[16], runs[17], runs[per - 1], runs[per] = per + 1, 0, 2, per + 1, 1, 0, per + 1
    run_concat(env, "concat %d blocks init %d" % (len(runs), with_init), runs, with_init, rng)
    run_concat(env, "concat passes init %d" % with_init, [short, short + 1, 0, pas + 3, 1], with_init, rng)
    run_concat(env, "concat one empty block init %d" % with_init, [0], with_init, rng)


# ===================================================================================================== pack
PACK = {"plain": ("PackPlain", 0, 0), "vlog": ("PackVlog", 8, 0), "sst": ("PackSst", 0, 5), "log": ("PackLog", 7, 0)}
PACK_LENGTHS = [0, 1, 15, 16, 17, 31, 33, 255, 4097]


def pack_batch(env, rng, lead, trail):
    """Blocks (list of segment lists), segment offsets / lengths, destination offsets.  Blocks 0 .. 255: one segment
    each, source start residue k % 16 crossed with destination residue k // 16, the listed lengths in rotation; then
    every listed length once more as a three-segment block with an empty segment at 1 << 40 in the middle; a block of
    two tiles; an empty block; a block whose frame misses the destination's end by one byte, and one at kSkip -- the
    segments of those two point at 1 << 40.  The first segment starts on the payload's first byte, the last one ends
    on its last; the destination ends with the last fitting block."""
    seg_off, seg_len, blocks, pos = [], [], [], 0

    def seg(n, residue=None, far=False):
        nonlocal pos
        if far:
            seg_off.append(FAR)
        else:
            if residue is not None and seg_off:
                pos += 32 + (residue - pos) % 16  # a gap of 32 .. 47 bytes: an over-read shows in it
            seg_off.append(pos)
            pos += n
        seg_len.append(n)
        return len(seg_len) - 1

    for k in range(256):
        n = PACK_LENGTHS[k % len(PACK_LENGTHS)] if k else 33
        blocks.append([seg(n, k % 16, far=(n == 0))])
    for n in PACK_LENGTHS:
        blocks.append([seg(n, 5, far=(n == 0)), seg(0, far=True), seg(n // 2 + 3, 11)])
    blocks.append([seg(env.const["pack_kTile"] + 777, 3), seg(4097, 9)])
    blocks.append([])
    unfit = [len(blocks), len(blocks) + 1]
    blocks.append([seg(100, far=True)])
    blocks.append([seg(17, far=True)])
    blocks.append([seg(255, 7), seg(1, 0)])  # the last fitting block, its last segment ends the payload
    total = [sum(seg_len[j] for j in b) for b in blocks]
    dst_off, at = [], 0
    for k, b in enumerate(blocks):
        if k in unfit:
            dst_off.append(None)
            continue
        at += 48 + ((k // 16) % 16 - at) % 16 if k else 0  # a gap of 48 .. 63 bytes that must stay unwritten
        dst_off.append(at)
        at += lead + total[k] + trail
    dst_bytes = at
    dst_off[unfit[0]] = dst_bytes - (lead + total[unfit[0]] + trail) + 1  # one byte short of fitting
    dst_off[unfit[1]] = SKIP
    first = np.zeros(len(blocks) + 1, np.uint64)
    first[1:] = np.cumsum([len(b) for b in blocks])
    return blocks, np.array(seg_off, np.uint64), np.array(seg_len, np.uint64), first, np.array(dst_off, np.uint64), \
        dst_bytes, pos, set(unfit)


def run_pack(env, form, skew):
    from kvsep import extend_host, mask, splitmix64_bytes
    struct_name, lead, trail = PACK[form]
    tag = "pack %s skew %d" % (form, skew)
    rng = np.random.default_rng(len(form))
    blocks, seg_off, seg_len, first, dst_off, dst_bytes, psize, unfit = pack_batch(env, rng, lead, trail)
    count = len(blocks)
    data = splitmix64_bytes(psize, 77, 0)
    payload = [b"".join(data[int(seg_off[j]):int(seg_off[j]) + int(seg_len[j])].tobytes() for j in b if seg_len[j])
               for b in blocks]
    crc = np.array([extend_host(0, p) for p in payload], np.uint32)
    types = rng.integers(1, 5, count).astype(np.uint8)
    if form == "sst":
        crc = np.array([mask(int(x)) for x in crc], np.uint32)  # the trailer word as it is stored
    c = Call(env, tag)
    geo = dict(ln.split()[:2] for ln in env._ask("pack", count, 4))
    grid, short_wgs, team = int(geo["crc32c_pack_kernel"]), int(geo["short_wgs"]), int(geo["team"])
    base = c.image(data, skew)
    v = dict(base=base, seg_off=c.input("seg_off", seg_off), seg_len=c.input("seg_len", seg_len),
             first=c.input("first", first), dst=c.output("dst", dst_bytes), dst_bytes=dst_bytes,
             dst_off=c.input("dst_off", dst_off), count=count, nseg=seg_len.size, short_wgs=short_wgs, team=team)
    if form != "plain":
        v["crc"] = c.input("crc", crc)
    if form in ("sst", "log"):
        v["types"] = c.input("types", types)
    kernel = "pack_" + form
    c.launch(kernel, grid, env.const_threads("pack"), c.E.struct_kernarg(
        ASM, K[kernel], os.path.join(CSRC, "crc32c_pack.inc"), "PackArgs", v))
    # (d) and (b): the bytewise gather with its frame, and exactly those bytes written
    exp, want = np.full(dst_bytes, 0xCC, np.uint8), np.zeros(dst_bytes, bool)
    for k, p in enumerate(payload):
        if k in unfit:
            continue
        m = mask(int(crc[k]))
        frame = {"plain": b"", "vlog": m.to_bytes(4, "little") + (len(p) & 0xFFFFFFFF).to_bytes(4, "little"), "sst": b"",
                 "log": m.to_bytes(4, "little") + (len(p) & 0xFFFF).to_bytes(2, "little") + bytes([types[k]])}[form]
        tail = bytes([types[k]]) + int(crc[k]).to_bytes(4, "little") if form == "sst" else b""
        rec = frame + p + tail
        at = int(dst_off[k])
        exp[at:at + len(rec)] = np.frombuffer(rec, np.uint8)
        want[at:at + len(rec)] = True
    _, _, wr = c.mem.touched(c.addr["dst"])
    diff = np.nonzero(wr != want)[0]
    assert not diff.size, "%s: dst write marks differ from the framed blocks' bytes at %s" % (tag, diff[:8])
    got = c.get("dst", np.uint8)
    assert np.array_equal(got, exp), "%s: dst differs at %s" % (tag, np.nonzero(got != exp)[0][:8])
    # (a): payload reads inside the naturally aligned 16-B granules that hold a byte of a segment of a block that fits
    region, pay, n = c.img
    _, rd, _ = c.mem.touched(region)
    allowed = np.zeros(rd.size + 16, bool)
    for k, b in enumerate(blocks):
        if k not in unfit:
            for j in b:
                if seg_len[j]:
                    a = pay + int(seg_off[j])
                    allowed[a // 16 * 16 - region:-(-(a + int(seg_len[j])) // 16) * 16 - region] = True
    bad = np.nonzero(rd & ~allowed[:rd.size])[0]
    assert not bad.size, "%s: payload read at offset %d, outside the 16-B granules of the copied segments" % (
        tag, int(bad[0]) - (pay - region))
    for name, size in (("first", 8), ("dst_off", 8), ("seg_len", 8)):
        assert c.reads(name, size).all(), "%s: %s not read in full" % (tag, name)
    c.check(partial_out=("dst",), granule_image=True)


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("form", list(PACK))
def test_pack(env, form, skew):
    run_pack(env, form, skew)
