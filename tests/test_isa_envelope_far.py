"""The memory envelope of the gather-copy, the log fill and the offsets pass with all traffic at and across 2^32 from
the base.  CPU only; the sibling of tests/test_isa_envelope_framing.py, whose harness, kernels table and references
this file uses.

There every payload, destination and offset lies within a few hundred KiB of its base, so a kernel that added a
position in 32 bits, or kept a running sum there, would still pass.  Here the `base` and `dst` arguments are addresses at
which nothing is mapped; what is mapped is one window each, around base + 2^32 and dst + 2^32, with bytes on both sides
of the line (wave_emu.Memory.alloc_at: the span in between is not allocated).  A position that lost its upper half
falls short of the window and is the emulator's "bad address"; one that wrapped inside the window shows in the write
marks or the bytes.

  * the offsets pass (tile_sum, tile_scan, write) from start = 2^32 - 3000: the device-computed dst_off cross 2^32 in
    the middle of a tile; its output array is handed to the gather-copy as it is;
  * crc32c_pack_kernel<PackPlain> and <PackVlog>: segments below, across and above base + 2^32, blocks written below,
    across and above dst + 2^32, the last one ending at dst_bytes; dropped blocks (kSkip) point at 1 << 40;
  * logw_fill_kernel with the rec_at / frag_first / scratch words a layout leaves for records that follow
    2^32 - 65,536 appended bytes: frag_at and the pad zeros cross 2^32, the records' off[] lie above it.

The checks are the existing ones: reads only in the 16-B granules that hold a byte of a copied segment, writes exactly
where the contract says, results equal to the host references, no scratch word read before it is written.
"""
import os

import numpy as np
import pytest

from framing_builders import ref_offsets
from test_isa_envelope_framing import (ASM, CSRC, FAR, FIRST, FULL, GUARD, K, LAST, M64, MIDDLE, SEEDS, SKIP, Call,
                                       env, ref_fragments)  # noqa: F401  (env: the module's fixture)

T32 = 1 << 32
SRC_BASE, DST_BASE = 1 << 44, 3 << 43  # the kernels' base / dst arguments: nothing is mapped at either
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 255, 700]


def window(c, name, kind, base, lo, nbytes, data=None):
    """A tracked region that holds [base + lo, base + lo + nbytes) between two guards, and nothing near base."""
    region = c.mem.alloc_at(base + lo - GUARD, GUARD + nbytes + GUARD, data=data, at=GUARD)
    c.kind[region] = (kind, name)
    c.addr[name], c.size[name] = region, GUARD + nbytes + GUARD
    return region


def far_batch(rng):
    """40 blocks of 1..3 segments laid from base + 2^32 - 2000 with gaps of 32..47 bytes (an over-read shows in them),
    so that the segments pass 2^32 about a third of the way; every fifth block is dropped and its segments point at
    1 << 40."""
    blocks, seg_off, seg_len, keep, pos = [], [], [], [], T32 - 2000
    for k in range(40):
        kept = k % 5 != 3
        b = []
        for j in range(1 + k % 3):
            n = LENGTHS[(k + 2 * j) % len(LENGTHS)]
            if kept and n:
                pos += 32 + (k - pos) % 16
                seg_off.append(pos)
                pos += n
            else:
                seg_off.append(FAR + (k << 20))
            seg_len.append(n)
            b.append(len(seg_len) - 1)
        blocks.append(b)
        keep.append(int(kept))
    first = np.zeros(len(blocks) + 1, np.uint64)
    first[1:] = np.cumsum([len(b) for b in blocks])
    lo = T32 - 2000
    assert lo < T32 < pos and any(o < T32 < o + n for o, n in zip(seg_off, seg_len) if o < FAR)
    return blocks, np.array(seg_off, np.uint64), np.array(seg_len, np.uint64), first, np.array(keep, np.uint8), lo, pos


@pytest.mark.parametrize("form", ["plain", "vlog"])
def test_offsets_then_pack_across_4gib(env, form):
    from kvsep import extend_host, mask, splitmix64_bytes
    lead = {"plain": 0, "vlog": 8}[form]
    tag = "far offsets + pack %s" % form
    rng = np.random.default_rng(len(form))
    blocks, seg_off, seg_len, first, keep, lo, hi = far_batch(rng)
    count, nseg, start = len(blocks), seg_len.size, T32 - 3000
    exp_off, end, nk, kept_segs = ref_offsets(seg_len, first, keep, None, lead, 0, start, M64, count)
    laid = exp_off[exp_off != np.uint64(SKIP)]
    assert (laid < T32).any() and (laid > T32).any() and end > T32
    dst_bytes = end  # the last kept block ends with the destination

    c = Call(env, tag)
    data = splitmix64_bytes(hi - lo, 91, 0)
    src = window(c, "payload", "in", SRC_BASE, lo, hi - lo, data)
    dst = window(c, "dst", "out", DST_BASE, start, end - start, np.full(end - start, 0xCC, np.uint8))
    # ---- the offsets pass: its dst_off array is the copy's
    geo = env.geometry("offsets", count)
    nt = geo[0][1]
    ov = dict(seg_len=c.input("seg_len", seg_len), first=c.input("first", first), keep=c.input("keep", keep), head=lead,
              tail=0, start=start, max_size=M64, count=count, nseg=nseg, dst_off=c.output("dst_off", 8 * count),
              end=c.output("end", 8), nkept=c.output("nkept", 8), ext=c.scratch("ext", 8 * count))
    ov.update(env.tile_words(c, count))
    oargs = c.sargs("offsets_tile_sum", "OffsetsArgs", ov)
    for kernel, grid, threads in geo:
        if kernel == "offsets_tile_scan_kernel":
            c.launch("offsets_tile_scan", grid, threads, c.pargs("offsets_tile_scan", [
                ov["tile_sum"], ov["tile_kept"], ov["tile_base"], ov["grand"], nt]))
        else:
            c.launch(kernel[:-7], grid, threads, oargs)
    got = c.get("dst_off", np.uint64)
    assert np.array_equal(got, exp_off), "%s: dst_off differs at %s" % (tag, np.nonzero(got != exp_off)[0][:8])
    assert int(c.get("end", np.uint64)[0]) == end and int(c.get("nkept", np.uint64)[0]) == nk, tag
    assert set(np.nonzero(c.reads("seg_len", 8))[0].tolist()) == kept_segs, tag
    # ---- the gather-copy
    payload = [b"".join(data[int(seg_off[j]) - lo:int(seg_off[j]) - lo + int(seg_len[j])].tobytes()
                        for j in b if seg_len[j]) if keep[k] else b"" for k, b in enumerate(blocks)]
    crc = np.array([extend_host(0, p) for p in payload], np.uint32)
    pgeo = dict(ln.split()[:2] for ln in env._ask("pack", count, 4))
    v = dict(base=SRC_BASE, seg_off=c.input("seg_off", seg_off), seg_len=ov["seg_len"], first=ov["first"], dst=DST_BASE,
             dst_bytes=dst_bytes, dst_off=ov["dst_off"], count=count, nseg=nseg, short_wgs=int(pgeo["short_wgs"]),
             team=int(pgeo["team"]))
    if form == "vlog":
        v["crc"] = c.input("crc", crc)
    kernel = "pack_" + form
    c.launch(kernel, int(pgeo["crc32c_pack_kernel"]), env.const_threads("pack"), c.E.struct_kernarg(
        ASM, K[kernel], os.path.join(CSRC, "crc32c_pack.inc"), "PackArgs", v))
    # (b) and (d): exactly the framed blocks' bytes written, and they are the bytewise gather
    size = c.size["dst"]
    exp, want = c.get("dst", np.uint8), np.zeros(size, bool)
    exp[:] = 0
    exp[GUARD:size - GUARD] = 0xCC
    for k, p in enumerate(payload):
        if not keep[k]:
            continue
        frame = mask(int(crc[k])).to_bytes(4, "little") + len(p).to_bytes(4, "little") if form == "vlog" else b""
        at = int(exp_off[k]) - start + GUARD
        exp[at:at + len(frame) + len(p)] = np.frombuffer(frame + p, np.uint8)
        want[at:at + len(frame) + len(p)] = True
    assert want[size - GUARD - 1] and not want[size - GUARD:].any()
    _, _, wr = c.mem.touched(dst)
    diff = np.nonzero(wr != want)[0]
    assert not diff.size, "%s: dst write marks differ from the framed blocks' bytes at %s (2^32 is at %d)" % (
        tag, diff[:8], T32 - start + GUARD)
    got = c.get("dst", np.uint8)
    assert np.array_equal(got, exp), "%s: dst differs at %s" % (tag, np.nonzero(got != exp)[0][:8])
    # (a): payload reads inside the naturally aligned 16-B granules that hold a byte of a copied segment
    _, rd, _ = c.mem.touched(src)
    allowed = np.zeros(rd.size + 16, bool)
    for k, b in enumerate(blocks):
        for j in b:
            if keep[k] and seg_len[j]:
                a = SRC_BASE + int(seg_off[j])
                allowed[a // 16 * 16 - src:-(-(a + int(seg_len[j])) // 16) * 16 - src] = True
    bad = np.nonzero(rd & ~allowed[:rd.size])[0]
    assert not bad.size, "%s: payload read at 2^32 %+d, outside the 16-B granules of the copied segments" % (
        tag, src + int(bad[0]) - SRC_BASE - T32)
    for name, width in (("first", 8), ("dst_off", 8), ("seg_len", 8)):
        assert c.reads(name, width).all(), "%s: %s not read in full" % (tag, name)
    c.check(partial_out=("dst",))


def test_log_fill_across_4gib(env):
    """logw_fill_kernel alone, on what logw_layout_kernel leaves for 40 records of up to 20,000 bytes that follow
    2^32 - 65,536 bytes appended by the same call (a multiple of the block size, so every block offset is that of
    kvsep_log_frame_layout for the records alone): rec_at, frag_at and the pad zeros cross 2^32."""
    from kvsep import log_frame_layout
    B, shift, dest_length = env.const["logw_kBlock"], T32 - 65536, 5 * 32768 + 32000
    rng = np.random.default_rng(40)
    ln = rng.integers(0, 20001, 40).astype(np.uint64)
    ln[7] = 0
    for i in (3, 11, 19, 30):  # records that leave 1..6 bytes in their block: the next one is led by pad zeros
        room, left = B - (dest_length + int(log_frame_layout(ln[:i], None, dest_length)[3])) % B, 1 + i % 6
        ln[i] = B - 7 - left if room < 7 else room - 7 - left if room - 7 - left >= 0 else room + B - 14 - left
    count = ln.size
    rec_at, frag_first, nfrag, written = log_frame_layout(ln, None, dest_length)
    b0 = dest_length % B
    frags, pads = ref_fragments(env, ln, [int(x) for x in rec_at], b0)
    assert len(frags) == nfrag and len(pads) >= 4
    frag_cap, dst_bytes = nfrag + 3, shift + written
    assert shift < T32 < shift + written - B
    rec = np.array([((int(a) + b0) % B) | ((pads[i][1] - pads[i][0] if i in pads else 0) << 16)
                    for i, a in enumerate(rec_at)], np.uint32)
    off = np.arange(count, dtype=np.uint64) * np.uint64(1 << 20) + np.uint64(T32 - 100)
    tag = "far logw fill"
    c = Call(env, tag)
    dst = window(c, "dst", "out", DST_BASE, shift, written, np.full(written, 0xCC, np.uint8))
    v = dict(len=c.input("len", ln), off=c.input("off", off), count=count, b0=b0, dst=DST_BASE, dst_bytes=dst_bytes,
             rec_at=c.input("rec_at", rec_at + np.uint64(shift)), frag_first=c.input("frag_first", frag_first),
             frag_off=c.output("frag_off", 8 * frag_cap), frag_len=c.output("frag_len", 8 * frag_cap),
             frag_at=c.output("frag_at", 8 * frag_cap), frag_type=c.output("frag_type", frag_cap), frag_cap=frag_cap,
             nfrag=c.input("nfrag", np.array([nfrag], np.uint64)), rec=c.input("rec", rec),
             seed=c.output("seed", 4 * frag_cap), s1=SEEDS[FULL], s2=SEEDS[FIRST], s3=SEEDS[MIDDLE], s4=SEEDS[LAST])
    (_, grid, threads), = [g for g in env.geometry("logw", count, frag_cap) if g[0] == "logw_fill_kernel"]
    c.launch("logw_fill", grid, threads, c.sargs("logw_fill", "LogwArgs", v))
    e_off, e_len, e_at = np.zeros(frag_cap, np.uint64), np.zeros(frag_cap, np.uint64), np.full(frag_cap, SKIP, np.uint64)
    e_type, e_seed = np.zeros(frag_cap, np.uint8), np.zeros(frag_cap, np.uint32)
    for f, (i, begin, take, at, ftype) in enumerate(frags):
        e_off[f], e_len[f], e_at[f], e_type[f], e_seed[f] = int(off[i]) + begin, take, at + shift, ftype, SEEDS[ftype]
    assert (e_at[:nfrag] < T32).any() and (e_at[:nfrag] > T32).any()
    for name, exp, dt in (("frag_off", e_off, np.uint64), ("frag_len", e_len, np.uint64), ("frag_at", e_at, np.uint64),
                          ("frag_type", e_type, np.uint8), ("seed", e_seed, np.uint32)):
        got = c.get(name, dt)
        assert np.array_equal(got, exp), "%s: %s differs at %s" % (tag, name, np.nonzero(got != exp)[0][:8])
    want = np.zeros(c.size["dst"], bool)
    for lo, hi in pads.values():
        want[GUARD + lo:GUARD + hi] = True
    assert want[:GUARD + T32 - shift].any() and want[GUARD + T32 - shift:].any()  # pad zeros on both sides of 2^32
    _, _, wr = c.mem.touched(dst)
    assert np.array_equal(wr, want), "%s: dst written at %s, pad zeros expected at %s" % (
        tag, np.nonzero(wr)[0][:8], np.nonzero(want)[0][:8])
    assert (c.get("dst", np.uint8)[want] == 0).all()
    c.check(partial_out=("dst",))
