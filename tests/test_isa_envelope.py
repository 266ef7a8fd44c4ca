"""The memory envelope of the shipped CRC kernels: they touch nothing the caller did not hand them.  CPU only.

The C ABI asks for no padding: blocks sit at any byte alignment and a payload may end on the last byte of a mapping.
tools/wave_emu.py runs the compiled gfx950 assembly with every byte of the emulated memory carrying a read and a write
mark, the payload inside a guard region at a chosen distance from a 4 KiB boundary, no slack behind it, and -- unlike
tests/test_isa_emulation.py, which runs one middle workgroup of a 256-workgroup grid -- EVERY workgroup of a grid of
one or two, so the workgroups that own block 0, the last block, the partial last group and the partial last sorted
window run, with their descriptor look-ahead and their staging of the following item.  Per run:

 a. every payload / guard byte read lies in a naturally aligned 16-B granule (absolute address) that holds a byte of a
    block of the batch (GRANULE: the cooperative kernel holds it at the 128-B line) -- blocks are
    laid out with gaps of 2048 + (i % 128) bytes, so a read past a block's end shows in the gap;
 b. a zero-length block is never dereferenced: one at off = the payload's size (the first guard byte) and one at
    off = 1 << 40 (unmapped: a read there is the emulator's "bad address"), both returning their init;
 c. the descriptor arrays (off, len, init, expect, and the plan's pstart / pblk) are regions of exactly count elements:
    a read past one is a "bad address" too;
 d. nothing is written but out[0 .. count) (every word of it), the verdict slots and the plan's scratch (partial, the
    work counter);
 e. the results equal the oracle and the verify form's slots carry the planted mismatches (a kernel that skipped work
    would pass a test of addresses alone).

The verify form runs as the captured form (verdict slots), so no arrival count depends on the grid.  Of the support
kernels that read caller memory, sst_verify_prep_kernel and verify_slots_reduce_kernel run the same way (the latter's
LDS reduction compiles to ds_read2_b64 / ds_read2st64_b64 / ds_write2st64_b64, which the emulator executes now).  The
layout, log and list kernels have the same check in tests/test_isa_envelope_framing.py.
"""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kv-separate_amd")
ASM = os.path.join(PKG, "build", "crc32c_device-hip-amdgcn-amd-amdhsa-gfx950.s")
sys.path.insert(0, os.path.join(PKG, "tools"))
sys.path.insert(0, PKG)

SORTED = "_ZN5kvsep27crc32c_narrow_sorted_kernelILi4ELb1ELi1024ELb%dENS_5ExactEEEvNS_10PiecesArgsE"
NARROW16 = "_ZN5kvsep20crc32c_narrow_kernelILi4ELb1ELi1024ELb0ELb1ENS_7LdsFullELb%dENS_5ExactEEEvNS_10PiecesArgsE"
NARROW8 = "_ZN5kvsep20crc32c_narrow_kernelILi4ELb1ELi512ELb1ELb1ENS_7LdsFullELb%dENS_5ExactEEEvNS_10PiecesArgsE"
CLAIM = "_ZN5kvsep26crc32c_narrow_claim_kernelILi4ELi512ELb%dELb1ELi8ELj3EEEvNS_10PiecesArgsE"
CLAIM16 = "_ZN5kvsep26crc32c_narrow_claim_kernelILi4ELi512ELb%dELb1ELi16ELj0EEEvNS_10PiecesArgsE"
COOP = "_ZN5kvsep25crc32c_narrow_coop_kernelILb%dELb0EEEvNS_10PiecesArgsE"
COOP_INIT = "_ZN5kvsep25crc32c_narrow_coop_kernelILb%dELb1EEEvNS_10PiecesArgsE"  # kInit: per-block initial CRCs
PIECES = "_ZN5kvsep20crc32c_pieces_kernelILb%dELb%dELi4ELb1ELb1ELi512ELb1ELb%dENS_5ExactEEEvNS_10PiecesArgsE"
COMBINE = "_ZN5kvsep21crc32c_combine_kernelILb%dEEEvNS_10PiecesArgsE"
WIDE = "_ZN5kvsep20crc32c_pieces_kernelILb0ELb0ELi4ELb1ELb1ELi512ELb1ELb%dENS_5ExactEEEvNS_10PiecesArgsE"  # unplanned
# label -> (template without inits, template with inits, threads per workgroup)
KERNELS = {"sorted": (SORTED, SORTED, 1024), "narrow16": (NARROW16, NARROW16, 1024), "narrow8": (NARROW8, NARROW8, 512),
           "claim": (CLAIM, CLAIM, 512), "claim16": (CLAIM16, CLAIM16, 512), "coop": (COOP, COOP_INIT, 512),
           "wide": (WIDE, WIDE, 512)}
# assertion (a)'s granule per kernel: 16 B is what the kernels' comments claim; 128 only for one DESIGN.md §2 names
GRANULE = {k: 16 for k in KERNELS}
GRANULE["planned"] = 16
# the cooperative kernel loads every lane of a block's row 0 (take(): `r < K ? rows + r * kRow : dummy`) and zeroes the
# chunks before the block's first 16-B boundary afterwards: up to 112 B before the block, inside the 128-B line that
# holds that boundary -- a line with block bytes in it, so no page the block does not touch
GRANULE["coop"] = 128
SKEWS = [0, 1, 15, 16, 113, 127, 4095]  # 4095: the payload's first byte is the last of its page
GUARD = 8192  # tracked bytes before and after the payload: an over-read of a whole 1 KiB row lands in them
EDGE_LENGTHS = [0, 1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1151, 1152, 1153,
                4096]
FAR = 1 << 40  # an offset no region of the emulated memory reaches


def place(ln, far=(), at_end=()):
    """Offsets of blocks of lengths ln: block 0 at payload byte 0, gap i (after block i) of 2048 + (i % 128) bytes (the
    start residues mod 128 vary), the last block ending on the payload's final byte.  The zero-length blocks `far` /
    `at_end` get off = 1 << 40 / off = the payload's size instead.  -> (off, payload size)"""
    ln = np.asarray(ln, np.uint64)
    off = np.zeros(ln.size, np.uint64)
    pos = 0
    for i in range(ln.size):
        off[i] = pos
        pos += int(ln[i]) + (2048 + i % 128 if i + 1 < ln.size else 0)
    assert ln[0] > 0 and ln[-1] > 0 and pos == int(off[-1] + ln[-1])
    for i in far:
        assert ln[i] == 0
        off[i] = FAR
    for i in at_end:
        assert ln[i] == 0
        off[i] = pos
    return off, pos


class Layout:
    def __init__(self, ln, hint, seed, splitmix64_bytes, mask, far=(), at_end=()):
        self.ln = np.asarray(ln, np.uint64)
        self.n = self.ln.size
        self.off, self.size = place(self.ln, far, at_end)
        self.hint = hint
        self.data = splitmix64_bytes(self.size, seed, 0)
        assert self.data.size == self.size
        self.init = np.random.default_rng(seed).integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32)
        # the oracle never sees the two special offsets: an empty block's CRC is its init wherever it points
        ooff = np.where(self.ln == 0, np.uint64(0), self.off)
        orc = load_oracle()
        self.exp = orc.batch(self.data, ooff, self.ln, None, threads=8)
        self.exp_init = orc.batch(self.data, ooff, self.ln, self.init, threads=8)
        assert all(self.exp_init[i] == self.init[i] for i in list(far) + list(at_end))
        self.plant = np.unique([0, self.n // 2, self.n - 1])  # the first and the last block among the mismatches
        self.stored = np.array([mask(int(x)) for x in self.exp_init], np.uint32)
        self.stored[self.plant] ^= 0x100


@pytest.fixture(scope="module")
def env():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-s", "-C", PKG, "asm"], stdout=subprocess.DEVNULL)
    import wave_emu
    from kvsep import mask, splitmix64_bytes
    rng = np.random.default_rng(23)
    L = {}
    # Edges: 75 blocks (9 whole groups and one of 3; one whole sorted window and one of 11).  The listed lengths, the
    # rest short; block 3 empty at 1 << 40, block 73 (in the partial last group) empty at the payload's end
    ln = rng.integers(1, 300, 75)
    rest = [x for x in EDGE_LENGTHS if x not in (0, 113, 1153)]
    free = [i for i in range(1, 73) if i != 3]
    ln[rng.permutation(free)[:len(rest)]] = rest
    ln[0], ln[74] = 113, 1153  # a partial head chunk at the payload's first byte, a partial tail chunk at its last
    ln[3] = ln[73] = 0
    assert set(EDGE_LENGTHS) <= set(int(x) for x in ln)
    L["edges"] = Layout(ln, 4096, 31, splitmix64_bytes, mask, far=(3,), at_end=(73,))
    # Understated hint: 131 blocks up to 256 B, hint 256, with blocks of 257..600 B -- longer than the hint, so
    # narrow_deferred and its 8 sub-ranges run -- at both ends of the payload and every 9th block between
    ln = rng.integers(0, 257, 131)
    over = np.arange(0, 131, 9).tolist() + [129, 130]
    ln[over] = rng.integers(257, 601, len(over))
    ln[130] = 600
    ln[5] = 0
    L["hint"] = Layout(ln, 256, 37, splitmix64_bytes, mask, far=(5,))
    # Wide, planned, 16 KiB pieces: around the split threshold 2P, a block of 3 pieces and a remainder, a long one; an
    # empty block past the end and a one-byte block between them
    K = 1024
    L["planned0"] = Layout([32 * K - 1, 32 * K, 0, 32 * K + 1, 1, 48 * K + 5, 100 * K], 0, 41, splitmix64_bytes, mask,
                           at_end=(2,))
    for k in (1, 2):
        P = (16 * K) << k
        L["planned%d" % k] = Layout([2 * P, 3 * P + 17], 0, 43 + k, splitmix64_bytes, mask)
    return wave_emu, wave_emu.dev_tables(), L


def nearest_block(addr, pay, lay):
    """The block (empty ones too, at their off) nearest to addr, as text."""
    def dist(i):
        a = pay + int(lay.off[i])
        return max(a - addr, addr - (a + max(int(lay.ln[i]), 1)) + 1, 0)
    i = min(range(lay.n), key=dist)
    a = pay + int(lay.off[i])
    return "block %d [0x%x, 0x%x) of %d B" % (i, a, a + int(lay.ln[i]), int(lay.ln[i]))


def emulate(E, lay, tag, fn, *args, **kw):
    """fn(*args, **kw), an emulator run with state=: its "bad address" (a load or store outside every region: past a
    descriptor array, or a dereferenced empty block at 1 << 40) fails the test with the array and element, or the
    block, that the address belongs to."""
    try:
        return fn(*args, **kw)
    except E.EmuError as e:
        st = kw["state"]
        m = re.search(r"bad address 0x([0-9a-f]+)", str(e))
        if not m or "mem" not in st:
            raise
        addr, f = int(m.group(1), 16), st["fields"]
        for k, size in (("off", 8), ("len", 8), ("init", 4), ("expect", 4), ("out", 4), ("pstart", 8), ("pblk", 4),
                        ("partial", 4)):
            if k in f and f[k] - 4096 <= addr < f[k] + st["mem"].find(f[k], 1)[0].size + 4096:
                where = "%s[%d] of a batch of %d blocks" % (k, (addr - f[k]) // size, lay.n)
                break
        else:
            where = "payload %+d, nearest %s" % (addr - f["base"], nearest_block(addr, f["base"], lay))
        raise AssertionError("%s: %s: %s" % (tag, e, where)) from e


def check_envelope(E, st, lay, granule, label):
    """Assertions (a) and (d) on the access marks a run left in st["mem"]."""
    mem, f = st["mem"], st["fields"]
    region, rsize, pay, psize = mem.payload
    assert (pay, psize) == (f["base"], lay.size)
    _, rd, wr = mem.touched(region)
    allowed = np.zeros(rsize + granule, bool)
    for i in range(lay.n):
        if lay.ln[i]:
            a = pay + int(lay.off[i])
            lo, hi = a // granule * granule, -(-(a + int(lay.ln[i])) // granule) * granule
            allowed[max(lo - region, 0):hi - region] = True
    bad = np.nonzero(rd & ~allowed[:rsize])[0]
    if bad.size:
        addr = region + int(bad[0])
        raise AssertionError(
            "%s: %d bytes read outside the %d-B granules of the batch's blocks; first at 0x%x = payload %+d, nearest "
            "%s (payload at 0x%x, %d bytes)" % (label, bad.size, granule, addr, addr - pay,
                                                nearest_block(addr, pay, lay), pay, psize))
    w = np.nonzero(wr)[0]
    assert w.size == 0, "%s: payload / guard written at 0x%x (payload at 0x%x)" % (label, region + int(w[0]), pay)
    scratch = {f[k] for k in ("out", "vslot", "partial", "work_counter") if k in f}
    for base, (_, wmarks) in mem.marks.items():
        if base not in scratch:
            w = np.nonzero(wmarks)[0]
            assert w.size == 0, "%s: write at 0x%x, outside out[] and the kernel's scratch" % (label, base + int(w[0]))
    _, _, wout = mem.touched(f["out"])
    assert wout.size == 4 * lay.n and wout.all(), "%s: out[] words not written: %s" % (
        label, np.nonzero(~wout.reshape(-1, 4).all(axis=1))[0])


def run_both_forms(E, tabs, lay, label, grid, skew):
    plain, with_init, threads = KERNELS[label]
    wgs = list(range(grid))
    image = dict(slack=0, guard=GUARD, skew=skew, track=True)
    tag = "%s skew %d" % (label, skew)
    st = {}
    out, written, _, _, _ = emulate(E, lay, tag + " plain", E.run_batch_kernel, ASM, plain % 0, threads, lay.data,
                                    lay.off, lay.ln, tabs, grid=grid, hint=lay.hint, wgs=wgs, state=st, **image)
    assert written.all() and np.array_equal(out, lay.exp), f"{tag}: {np.count_nonzero(out != lay.exp)} wrong CRCs"
    check_envelope(E, st, lay, GRANULE[label], tag + " plain")
    # the verify form as captured, with per-block initial CRCs: init[] and expect[] join the descriptor arrays
    st = {}
    out, written, fb, nb, _ = emulate(E, lay, tag + " verify", E.run_batch_kernel, ASM, with_init % 1, threads,
                                      lay.data, lay.off, lay.ln, tabs, grid=grid, hint=lay.hint, wgs=wgs, state=st,
                                      init=lay.init, expect=lay.stored, vslot=True, **image)
    assert written.all() and np.array_equal(out, lay.exp_init), f"{tag}: wrong CRCs (verify form, inits)"
    assert (fb, nb) == (E.SENTINEL, E.SENTINEL)  # the captured form leaves the caller's words to the reduce kernel
    sl = st["slots"]
    assert len(sl) == grid and all(v != (E.SENTINEL, E.SENTINEL) for v in sl), sl
    assert (min(v[0] for v in sl), sum(v[1] for v in sl)) == (int(lay.plant.min()), lay.plant.size), sl
    check_envelope(E, st, lay, GRANULE[label], tag + " verify")


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("label", list(KERNELS))
def test_edges(env, label, skew):
    """The edge lengths at every skew, a grid of one workgroup: it owns every block, the partial last group / window."""
    E, tabs, L = env
    run_both_forms(E, tabs, L["edges"], label, 1, skew)


@pytest.mark.parametrize("label", list(KERNELS))
def test_understated_hint(env, label):
    """Blocks over the hint at both ends of the payload (narrow_deferred's 8 sub-ranges; the coop kernel's wide
    machinery), both workgroups of a grid of two; the payload's first byte last in its page."""
    E, tabs, L = env
    lay = L["hint"]
    assert lay.ln[0] > lay.hint and lay.ln[-1] > lay.hint
    run_both_forms(E, tabs, lay, label, 2, 4095)


def run_planned(E, tabs, lay, piece_k, skew, verify):
    image = dict(slack=0, guard=GUARD, skew=skew, track=True)
    tag = "planned piece_k %d skew %d verify %d" % (piece_k, skew, verify)
    st = {}
    grid = 2
    out, written, fb, nb, _ = emulate(
        E, lay, tag, E.run_planned_batch, ASM, PIECES % (1, 1, verify), COMBINE % verify, lay.data, lay.off, lay.ln,
        tabs, piece_k=piece_k, grid=grid, expect=_stored_plain(lay) if verify else None, state=st,
        pieces_wgs=range(grid), captured=bool(verify), **image)
    assert written.all() and np.array_equal(out, lay.exp), f"{tag}: {np.count_nonzero(out != lay.exp)} wrong CRCs"
    if verify:
        assert (fb, nb) == (E.SENTINEL, E.SENTINEL)
        sl = [v for v in st["slots"] if v != (E.SENTINEL, E.SENTINEL)]
        assert (min(v[0] for v in sl), sum(v[1] for v in sl)) == (int(lay.plant.min()), lay.plant.size), st["slots"]
    check_envelope(E, st, lay, GRANULE["planned"], tag)


def _stored_plain(lay):
    """Stored words for the batch without inits (the planned path's runs), the same planted blocks."""
    from kvsep import mask
    s = np.array([mask(int(x)) for x in lay.exp], np.uint32)
    s[lay.plant] ^= 0x100
    return s


@pytest.mark.parametrize("verify", [0, 1])
@pytest.mark.parametrize("skew", [1, 4095])
def test_wide_planned(env, skew, verify):
    """The split path: piece table, the wide kernel's guided schedule over both workgroups of its grid, the combine
    kernel; 16 KiB pieces, lengths around the split threshold."""
    E, tabs, L = env
    run_planned(E, tabs, L["planned0"], 0, skew, verify)


@pytest.mark.parametrize("piece_k,verify", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_wide_planned_larger_pieces(env, piece_k, verify):
    """zsmall[1] / zsmall[2] (32 and 64 KiB pieces): one block of 2P and one of 3P + 17."""
    E, tabs, L = env
    run_planned(E, tabs, L["planned%d" % piece_k], piece_k, 113, verify)


PREP = "_ZN5kvsep22sst_verify_prep_kernelEPKhPKmS3_PmPjm"


@pytest.mark.parametrize("skew", [0, 1, 4093, 4095])
def test_sst_verify_prep(env, skew):
    """The SST read side's prep kernel (len1 = len + 1, stored = the trailer's LE32 at off + len + 1 .. + 4): 259 blocks
    (two workgroups, the second with 3 threads in the batch), block 0 at payload byte 0, the last trailer ending on the
    payload's final byte.  It reads exactly the four trailer bytes of each block -- one unaligned dword load -- and the
    count elements of off / len, and writes len1 / stored only."""
    E, tabs, _ = env
    from kvsep import splitmix64_bytes
    rng = np.random.default_rng(47)
    n = 259
    ln = rng.integers(0, 200, n).astype(np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1] + np.uint64(5) + (np.uint64(2048) + np.arange(n - 1, dtype=np.uint64) % np.uint64(128)))
    size = int(off[-1] + ln[-1]) + 5
    data = splitmix64_bytes(size, 53, 0)
    mem, f = E.batch_memory(data, off, ln, tabs, slack=0, guard=GUARD, skew=skew, track=True)
    d_len1 = mem.alloc(8 * n, data=np.full(n, E.SENTINEL, np.uint64))
    d_stored = mem.alloc(4 * n, data=np.full(n, E.SENTINEL, np.uint32))
    args = struct.pack("<6Q", f["base"], f["off"], f["len"], d_len1, d_stored, n)
    try:
        E.launch_plain(mem, ASM, PREP, 256, args, (n + 255) // 256)
    except E.EmuError as e:
        raise AssertionError("sst_verify_prep skew %d: %s (off[] at 0x%x, len[] at 0x%x, %d blocks, payload at 0x%x)" %
                             (skew, e, f["off"], f["len"], n, f["base"])) from e
    trailer = np.array([int.from_bytes(data[int(o + l) + 1:int(o + l) + 5].tobytes(), "little")
                        for o, l in zip(off, ln)], np.uint32)
    assert np.array_equal(mem.view(d_len1, 8 * n).view(np.uint64), ln + np.uint64(1))
    assert np.array_equal(mem.view(d_stored, 4 * n).view(np.uint32), trailer)
    region, rsize, pay, psize = mem.payload
    _, rd, wr = mem.touched(region)
    want = np.zeros(rsize, bool)
    for o, l in zip(off, ln):
        a = pay - region + int(o + l) + 1
        want[a:a + 4] = True
    bad = np.nonzero(rd != want)[0]
    if bad.size:
        addr = region + int(bad[0])
        blk = int(np.argmin(np.abs((off + ln).astype(np.int64) + pay - addr)))
        raise AssertionError("sst_verify_prep skew %d: payload reads differ from the trailer words at 0x%x = payload "
                             "%+d, nearest trailer: block %d at 0x%x" % (skew, addr, addr - pay, blk,
                                                                        pay + int(off[blk] + ln[blk]) + 1))
    assert not wr.any()
    for base, (_, wmarks) in mem.marks.items():
        assert wmarks.all() if base in (d_len1, d_stored) else not wmarks.any(), "write at region 0x%x" % base


REDUCE = "_ZN5kvsep26verify_slots_reduce_kernelEPKyjPyS2_"


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700])
@pytest.mark.parametrize("clean", [False, True])
def test_verify_slots_reduce(env, n, clean):
    """The captured verify call's verdict: the lowest bad block and the total over n (lowest, count) slots, one workgroup
    of 256.  vslot is a region of exactly n pairs (n = 0: an unmapped address) and is read in full and never written;
    the two verdict words are written in full.  A slot with count 0 holds the sentinel pair's "none" as its block."""
    E, _, _ = env
    rng = np.random.default_rng(n)
    slot = np.zeros((n, 2), np.uint64)
    slot[:, 0] = ~np.uint64(0)
    if not clean and n:
        hit = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 5)]))
        slot[hit, 0] = rng.integers(1 << 33, 1 << 40, hit.size).astype(np.uint64)
        slot[hit, 1] = rng.integers(1, 1000, hit.size).astype(np.uint64)
    mem = E.Memory(track=True)
    d_slot = mem.alloc(16 * n, data=slot) if n else 1 << 40
    d_fb = mem.alloc(8, data=np.array([E.SENTINEL], np.uint64))
    d_nb = mem.alloc(8, data=np.array([E.SENTINEL], np.uint64))
    try:
        steps = E.launch_args(mem, ASM, REDUCE, 256, E.args_kernarg(ASM, REDUCE, [d_slot, n, d_fb, d_nb]), 1)
    except E.EmuError as e:
        raise AssertionError("verify_slots_reduce n %d: %s (vslot at 0x%x, %d bytes)" % (n, e, d_slot, 16 * n)) from e
    print("verify_slots_reduce n %d: %d wave-instructions" % (n, steps))
    total = int(slot[:, 1].sum())
    assert mem.peek64(d_nb) == total
    assert mem.peek64(d_fb) == (int(slot[:, 0].min()) if total else (1 << 64) - 1)
    for base, (rd, wr) in mem.marks.items():
        if base == d_slot:
            assert rd.all() and not wr.any()
        elif base in (d_fb, d_nb):
            assert wr.all() and not rd.any()
