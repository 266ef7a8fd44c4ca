#!/usr/bin/env python3
"""Seeded differential soak of the list, combine, frame, layout, log-read, log-write, SST-read and SST-write device forms,
and of mixed sequences of them on one context: the sibling of soak.py for what was built since round 6.

Three layers; the first two need no GPU and never touch torch.cuda:
  generators  make_case(family, seed, index): inputs, call parameters, a one-line description and the edge classes the
              case reaches.  A case depends on (family, seed, index) alone, so any reported case is rebuilt and run by
              itself with --family F --seed S --case K.
  models      expect(case): every output array and every destination byte the device call must produce, as plain serial
              Python / numpy over the oracle's CRC (tests/conftest.load_oracle) and the restatements of
              tests/framing_builders.py and tests/sst_tables.py.  No *_run.h rule and no kvsep host form is consulted.
  runner      run_case(ctx, case, stream): uploads, calls, downloads.  Every output array lies between guard elements,
              every destination between 64 canary bytes; compare() checks every element, the guards and that the inputs
              are unchanged, and names the family, seed, case, array and index of the first difference.

What the soak does not reach: a case holds at most MAX_ELEMENTS elements and MAX_PAYLOAD (8 MiB) of payload, so that it
stays fast; every position it produces is far below 2^32 (a far `start` or dest_length enters as arithmetic only).
Offsets and totals of 2^32 and over -- far seg_off / dst_off / rec_off, sums and payloads that pass 4 GiB, a log image
over 4 GiB -- are covered by tests/test_gpu_far_offsets.py, which uses the models below, and by
tests/test_isa_envelope_far.py on the shipped assembly.

usage: soak_forms.py [--seconds 240] [--seed N] [--family F] [--case K]
One line per case; exits non-zero on the first mismatch.  tests/test_gpu_soak_forms.py runs a fixed seeded slice,
tests/test_soak_forms_cpu.py checks the models against the host forms, the generators' reach and the comparator."""
import argparse
import copy
import os
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
import numpy as np  # noqa: E402

import framing_builders as FB  # noqa: E402
import sst_tables as T  # noqa: E402
from conftest import load_oracle  # noqa: E402  (the checker)
from kvsep import splitmix64_bytes  # noqa: E402

U64 = 0xFFFFFFFFFFFFFFFF
SKIP = U64
CANARY = 0xA5
G = 8      # guard elements on each side of an output array
DG = 64    # guard bytes on each side of a destination
SKEW = 16  # room for a destination's base skew
MAX_ELEMENTS = 4200
MAX_PAYLOAD = 8 << 20
MASK_DELTA = 0xA282EAD8
SST_OK, SSTW_OK, SSTW_NO_ROOM = 0, 0, 2
SST_BAD_FOOTER, SST_INDEX_CHECKSUM, SST_INDEX_COMPRESSED, SST_CAP, SST_SHARED_KEY = 1, 2, 3, 7, 8

FAMILIES = ("lists", "combine", "frame", "layout", "logread", "logwrite", "sstread", "sstwrite", "sequence",
            "captured")
FAMILY_ID = {f: i for i, f in enumerate(FAMILIES)}
SINGLE = FAMILIES[:8]

_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = load_oracle()
    return _ORACLE


def mask32(crc):
    """leveldb::crc32c::Mask over a uint32 array (util/crc32c.h:29)."""
    c = np.asarray(crc, np.uint64)
    return ((((c >> np.uint64(15)) | (c << np.uint64(17))) + np.uint64(MASK_DELTA)) & np.uint64(0xFFFFFFFF)).astype(
        np.uint32)


def mask1(crc):
    return int(oracle().lib.oracle_crc32c_mask(int(crc) & 0xFFFFFFFF))


class Mismatch(AssertionError):
    def __init__(self, msg, array=None, index=None):
        super().__init__(msg)
        self.array, self.index = array, index


class Case:
    """inp: the arrays that are uploaded (an absent optional one is passed as a null pointer); host: what only the
    model reads; par: scalars of the call; out: name -> (dtype, elements) of every output array ("dst" is the
    destination of par["dst_bytes"] bytes at skew par["dst_skew"]); edges: the edge classes this case reaches."""

    def __init__(self, family, seed, index):
        self.family, self.seed, self.index = family, seed, index
        self.form, self.desc = "", ""
        self.inp, self.host, self.par, self.out = {}, {}, {}, {}
        self.edges = set()
        self.elements = self.nbytes = 0
        self.members = []  # the sequence families
        self.refused = None  # captured: a call captured over its reservation

    @property
    def id(self):
        return f"{self.family}/{self.seed}/{self.index}"

    def line(self):
        return f"{self.id} {self.form}: {self.desc}"


# ====================================================================================================== generators
def draw_count(rng, hi=MAX_ELEMENTS):
    """Counts around the 64-lane, 256-lane and 1,024-tile edges, mostly small."""
    r = rng.random()
    if r < 0.45:
        return int(rng.choice([0, 1, 2, 63, 64, 65, 255, 256, 257]))
    if r < 0.6:
        return min(hi, int(rng.choice([1023, 1024, 1025, 2049, 4200])))
    if r < 0.9:
        return int(rng.integers(0, min(hi, 300) + 1))
    return int(rng.integers(0, hi + 1))


def count_edges(c, n):
    c.elements = max(c.elements, n)
    if n == 0:
        c.edges.add("count0")
    if n == 1:
        c.edges.add("count1")
    if 1025 <= n <= MAX_ELEMENTS:
        c.edges.add("count_big")


def draw_lengths(rng, n, budget=MAX_PAYLOAD // 2, tops=(0, 8, 300, 5000)):
    top = int(rng.choice(tops))
    ln = rng.integers(0, top + 1, n).astype(np.uint64)
    if n and rng.random() < 0.3:
        ln[rng.random(n) < 0.2] = 0
    while int(ln.sum()) > budget:
        ln //= np.uint64(2)
    return ln


def pool(c, nbytes, salt=0):
    """A source of nbytes pseudo-random bytes at base + skew (0..15): inp["src"] holds skew bytes in front."""
    rng = c.host["rng"]
    skew = int(rng.integers(0, 16))
    if skew:
        c.edges.add("skew")
    c.par["src_skew"] = skew
    c.inp["src"] = splitmix64_bytes(nbytes + skew, (c.seed * 1000003 + c.index * 7 + salt) & U64, 0)
    c.nbytes += nbytes
    return c.inp["src"][skew:]


def scatter(rng, ln, span):
    """Offsets anywhere in [0, span): out of order, overlapping, any alignment."""
    ln = ln.astype(np.int64)
    return (rng.integers(0, 1 << 62, ln.size) % (span + 1 - ln)).astype(np.uint64)


def draw_hint(rng, ln):
    mx = int(ln.max()) if ln.size else 0
    return int(rng.choice([0, mx, 2 * mx + 1]))


def draw_dst(c, rng, need, refusal="dst_short"):
    """The destination: exactly `need` bytes, one byte short or (so that a write past the end has somewhere to show)
    a few bytes more, at a skew of 0..15."""
    r = rng.random()
    short = need > 0 and r < 0.3
    if short:
        c.edges.add("refusal:" + refusal)
    c.par["dst_bytes"] = need - 1 if short else need + int(rng.integers(1, 65)) if r > 0.8 else need
    c.par["dst_skew"] = int(rng.integers(0, 16))
    if c.par["dst_skew"]:
        c.edges.add("dst_skew")
    c.out["dst"] = (np.uint8, c.par["dst_bytes"])
    return short


def sst_file(c, rng, n, ln):
    """[block][type][Mask(Value(block || type)) LE32] at each handle, gaps between them -> (image, positions)."""
    gaps = rng.integers(0, 4, n).astype(np.uint64)
    pos = np.zeros(n, np.uint64)
    if n:
        pos[1:] = np.cumsum(ln[:-1] + np.uint64(5) + gaps[:-1], dtype=np.uint64)
    size = int(pos[-1] + ln[-1]) + 5 if n else 0
    img = pool(c, size + 3)
    if n:
        p = pos.astype(np.int64)
        img[p + ln.astype(np.int64)] = rng.integers(0, 2, n).astype(np.uint8)
        word = mask32(oracle().batch(img, pos, ln + np.uint64(1)))
        for k in range(4):
            img[p + ln.astype(np.int64) + 1 + k] = ((word >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint8)
    return img, pos


def bad_fraction(rng, n):
    f = float(rng.choice([0.0, -1.0, 0.01, 0.33, 1.01]))
    if f < 0:  # one or two blocks
        bad = np.zeros(n, bool)
        if n:
            bad[rng.integers(0, n, 2)] = True
        return bad
    return rng.random(n) < f


def gen_lists(c, rng):
    n = draw_count(rng)
    count_edges(c, n)
    ln = draw_lengths(rng, n)
    c.form = str(rng.choice(["verify_list", "sst_verify_list"]))
    bad = bad_fraction(rng, n)
    if c.form == "verify_list":
        span = max(int(ln.sum()) // 2, int(ln.max()) if n else 0, 64)
        src = pool(c, span)
        off = scatter(rng, ln, span)
        init = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) if rng.random() < 0.5 else None
        word = mask32(oracle().batch(src, off, ln, init))
        word[bad] ^= np.uint32(1 << int(rng.integers(0, 32)))
        c.inp.update(off=off, len=ln, expected=word)
        if init is not None:
            c.inp["init"] = init
    else:
        img, pos = sst_file(c, rng, n, ln)
        for i in np.flatnonzero(bad):  # a payload byte, the type byte or a trailer byte
            img[int(pos[i]) + int(rng.integers(0, int(ln[i]) + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        c.inp.update(off=pos, len=ln)
    nbad = int(bad.sum())
    kind = str(rng.choice(["below", "at", "above"]))
    cap = max(0, nbad + {"below": -1, "at": 0, "above": 3}[kind])
    c.edges.add("cap_" + kind)
    c.edges.add("bad_none" if nbad == 0 else "bad_all" if nbad == n else "bad_some")
    with_ok = bool(rng.random() < 0.5)
    c.edges.add("ok" if with_ok else "no_ok")
    c.par.update(count=n, bad_cap=cap, max_len=draw_hint(rng, ln), total=int(ln.sum()))
    c.out.update(out=(np.uint32, n), first_bad=(np.uint64, 1), nbad=(np.uint64, 1))
    if cap:
        c.out["bad_idx"] = (np.uint64, cap)
    if with_ok:
        c.out["ok"] = (np.uint8, n)
    c.desc = f"n={n} bad={nbad} cap={cap} ok={int(with_ok)} hint={c.par['max_len']}"


def clip_runs(runs, budget=MAX_ELEMENTS):
    """What does not fit the element limit is cut short (the runs after it are empty), never dropped afterwards."""
    out, used = [], 0
    for r in runs:
        r = min(int(r), budget - used)
        out.append(r)
        used += r
    return np.array(out, np.int64).reshape(len(out))


def draw_runs(rng):
    """Segment runs around the short / long threshold of 32, empty runs, and one long run now and then."""
    runs = []
    nblocks = draw_count(rng, MAX_ELEMENTS - 1)
    if rng.random() < 0.2:
        runs.append(int(rng.choice([1024, 1025, 4096, 4097])))
    for _ in range(nblocks):
        runs.append(int(rng.choice([0, 1, 2, 5, 31, 32, 33, 40])) if rng.random() < 0.8 else int(rng.integers(0, 80)))
    order = rng.permutation(len(runs))
    return clip_runs([runs[i] for i in order])


def gen_combine(c, rng):
    runs = draw_runs(rng)
    n, nseg = runs.size, int(runs.sum())
    count_edges(c, max(n, nseg))
    count_edges(c, n)
    for r in (31, 32, 33):
        if (runs == r).any():
            c.edges.add(f"run{r}")
    if (runs == 0).any():
        c.edges.add("run_empty")
    ln = draw_lengths(rng, nseg)
    if nseg and (ln == 0).any():
        c.edges.add("seg_empty")
    span = max(int(ln.sum()) // 2, int(ln.max()) if nseg else 0, 64)
    c.form = str(rng.choice(["concat", "gather"]))
    src = pool(c, span)
    off = scatter(rng, ln, span)
    first = np.zeros(n + 1, np.uint64)
    first[1:] = np.cumsum(runs)
    if n > 1 and rng.random() < 0.1:  # values past nseg and runs that end before they start: clamped, empty
        k = rng.integers(0, n + 1, 3)
        first[k] = rng.integers(0, nseg + 9, 3).astype(np.uint64)
        c.edges.add("first_wild")
    c.inp.update(seg_len=ln, first=first)
    if rng.random() < 0.5:
        c.inp["init"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        c.edges.add("init")
    else:
        c.edges.add("no_init")
    c.par.update(count=n, nseg=nseg, max_len=draw_hint(rng, ln), total=int(ln.sum()))
    c.out["out"] = (np.uint32, n)
    if c.form == "concat":  # no payload on the device: the segments' CRCs go in
        c.host.update(src=src.copy(), seg_off=off)
        c.inp["seg_crc"] = oracle().batch(src, off, ln)
        del c.inp["src"]
    else:
        c.inp["seg_off"] = off
        c.out["seg_crc"] = (np.uint32, nseg)
    c.desc = f"blocks={n} nseg={nseg} longest run={int(runs.max()) if n else 0} init={int('init' in c.inp)}"


def gen_frame(c, rng):
    c.form = str(rng.choice(["pack", "vlog_frame", "vlog_frame_auto", "sst_frame"]))
    top = int(rng.choice([0, 40, 300, 5000, 70000]))
    n = draw_count(rng, MAX_ELEMENTS if top <= 300 else 60 if top == 5000 else 12)
    runs = np.ones(n, np.int64) if c.form == "sst_frame" else clip_runs(rng.integers(1, 9, n))
    nseg = int(runs.sum())
    count_edges(c, max(n, nseg))
    count_edges(c, n)
    ln = rng.integers(0, top + 1, nseg).astype(np.uint64)
    if nseg and rng.random() < 0.3:
        ln[rng.random(nseg) < 0.2] = 0
    if top >= 4096 and nseg:
        c.edges.add("long_segment")
    span = max(min(int(ln.sum()), 1 << 20), int(ln.max()) if nseg else 0, 64)
    pool(c, span)
    off = scatter(rng, ln, span)
    first = np.zeros(n + 1, np.uint64)
    first[1:] = np.cumsum(runs)
    size = np.array([int(ln[int(first[i]):int(first[i + 1])].sum()) for i in range(n)], np.uint64)
    frame = {"pack": 0, "vlog_frame": 8, "vlog_frame_auto": 8, "sst_frame": 5}[c.form]
    start = int(rng.choice([0, int(rng.integers(0, 1000))])) if c.form == "vlog_frame_auto" else 0
    # records back to back (with gaps of 0..3 where the caller chooses the offsets), laid out in a shuffled order
    order = rng.permutation(n) if c.form != "vlog_frame_auto" and rng.random() < 0.5 else np.arange(n)
    gap_top = 1 if c.form == "vlog_frame_auto" or rng.random() < 0.5 else 4
    at, p = np.zeros(n, np.uint64), start
    for i in order:
        p += int(rng.integers(0, gap_top))
        at[i] = p
        p += frame + int(size[i])
    draw_dst(c, rng, p)
    c.par.update(count=n, nseg=nseg, max_len=draw_hint(rng, ln), total=int(ln.sum()), start=start)
    if c.form == "sst_frame":
        c.inp.update(off=off, len=ln, types=rng.integers(0, 2, n).astype(np.uint8), blk_off=at)
        c.out["masked_out"] = (np.uint32, n)
    else:
        c.inp.update(seg_off=off, seg_len=ln, first=first)
        if c.form != "vlog_frame_auto":
            c.inp["dst_off"] = at
        else:
            c.out.update(rec_off=(np.uint64, n), end=(np.uint64, 1))
        if c.form != "pack":
            c.out.update(seg_crc=(np.uint32, nseg), crc_out=(np.uint32, n))
    c.desc = (f"records={n} nseg={nseg} top={top} skews={c.par['src_skew']}/{c.par['dst_skew']} start={start} "
              f"dst={c.par['dst_bytes']}/{p}")


def draw_keep(c, rng, n):
    """One of the three keep rules -> (keep array or None, keep_before or None)."""
    rule = str(rng.choice(["all", "keep", "before"]))
    c.edges.add("rule_" + rule)
    if rule == "keep":
        f = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.01]))
        c.inp["keep"] = (rng.random(n) < f).astype(np.uint8) * np.uint8(rng.choice([1, 0x80]))
    elif rule == "before":
        c.inp["keep_before"] = np.array([[0, n // 2, max(n - 1, 0), n, n + 5, U64][int(rng.integers(0, 6))]], np.uint64)


def gen_layout(c, rng):
    c.form = str(rng.choice(["offsets", "salvage", "sst_salvage"]))
    n = draw_count(rng)
    count_edges(c, n)
    if c.form == "offsets":
        with_first = bool(rng.random() < 0.5)
        runs = clip_runs(rng.integers(0, 5, n)) if with_first else np.ones(n, np.int64)
        nseg = int(runs.sum())
        ln = draw_lengths(rng, nseg, tops=(0, 8, 300, 70000))
        head, tail = (int(rng.choice([0, 5, 8, 1 << 20])) for _ in range(2))
        start = [0, 7, 1 << 33][int(rng.integers(0, 3))]
        if nseg and rng.random() < 0.35:  # sums that saturate: a length near 2^64, KVSEP_OFFSET_SKIP as a length, a far start
            how = str(rng.choice(["huge", "skip", "two_halves", "start"]))
            k = rng.integers(0, nseg, 2)
            if how == "huge":
                ln[k[0]] = np.uint64(U64 - int(rng.integers(1, 4096)))
            elif how == "skip":
                ln[k[0]] = np.uint64(SKIP)
            elif how == "two_halves":
                ln[k] = np.uint64(1 << 63)
            else:
                start = U64 - int(rng.integers(0, 64))
            c.edges.add("huge_" + how)
        if with_first:
            first = np.zeros(n + 1, np.uint64)
            first[1:] = np.cumsum(runs)
            c.inp["first"] = first
            c.edges.add("first")
        c.inp["seg_len"] = ln
        draw_keep(c, rng, n)
        c.par.update(count=n, nseg=nseg, head=head, tail=tail, start=start)
        c.out.update(dst_off=(np.uint64, n), end=(np.uint64, 1), nkept=(np.uint64, 1))
        c.elements = max(n, nseg)
        c.desc = f"n={n} nseg={nseg} head={head} tail={tail} start={start}"
        return
    ln = draw_lengths(rng, n, tops=(0, 40, 300, 5000))
    if c.form == "salvage":
        span = max(min(int(ln.sum()), 1 << 20), int(ln.max()) if n else 0, 64)
        pool(c, span)
        off = scatter(rng, ln, span)
        draw_keep(c, rng, n)
        kept = np.ones(n, bool)
        if "keep" in c.inp:
            kept = c.inp["keep"] != 0
        if "keep_before" in c.inp:
            kept = np.arange(n, dtype=np.uint64) < c.inp["keep_before"][0]
        need = int(ln[kept].sum())
    else:
        img, off = sst_file(c, rng, n, ln)
        bad = bad_fraction(rng, n)
        for i in np.flatnonzero(bad):
            img[int(off[i]) + int(rng.integers(0, int(ln[i]) + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        need = int((ln[~bad] + np.uint64(5)).sum())  # (a flipped bit does not leave a block's checksum good)
        c.par.update(max_len=draw_hint(rng, ln), total=int(ln.sum()))
        c.out.update(out=(np.uint32, n), first_bad=(np.uint64, 1), nbad=(np.uint64, 1), ok=(np.uint8, n))
    c.inp.update(off=off, len=ln)
    draw_dst(c, rng, need)
    c.par["count"] = n
    c.out.update(dst_off=(np.uint64, n), end=(np.uint64, 1), nkept=(np.uint64, 1))
    c.desc = f"n={n} need={need} dst={c.par['dst_bytes']} skews={c.par['src_skew']}/{c.par['dst_skew']}"


DAMAGES = ("payload", "crc", "length", "type", "zero_block", "truncate")


def draw_records(c, rng, n, style, pos, budget=60 * FB.BLOCK):
    """Record lengths of 0..100,000 bytes, among them ones that leave 0..7 bytes in their block."""
    lens = []
    for _ in range(n):
        if style == "tiny":
            k = int(rng.integers(0, 41))
        elif style == "edge" and rng.random() < 0.5:
            k = (FB.BLOCK - pos - FB.HEADER - int(rng.integers(0, 8))) % FB.BLOCK
            c.edges.add("block_tail")
        elif style == "long" and rng.random() < 0.4:
            k = int(rng.integers(30000, 100001))
        else:
            k = int(rng.integers(0, 5000))
        k = max(0, min(k, budget))
        budget -= k + 2 * FB.HEADER
        lens.append(k)
        pos = (pos + k + FB.HEADER) % FB.BLOCK  # an estimate of the writer's position: it only steers the draw
    return lens


def damage(c, rng, img, phys, kind):
    """One damage of a log image in place (truncate: -> the new length)."""
    inside = [p for p in phys if p[0] + FB.HEADER + p[2] <= len(img)]
    if kind == "truncate":
        c.edges.add("damage_truncate")
        return int(rng.integers(0, len(img) + 1))
    if kind == "zero_block":
        if len(img):
            b = int(rng.integers(0, (len(img) + FB.BLOCK - 1) // FB.BLOCK)) * FB.BLOCK
            img[b:b + FB.BLOCK] = bytes(len(img[b:b + FB.BLOCK]))
            c.edges.add("damage_zero_block")
        return len(img)
    if kind == "payload":
        inside = [p for p in inside if p[2]]
    if not inside:
        return len(img)
    at, t, k = inside[int(rng.integers(0, len(inside)))]
    bit = 1 << int(rng.integers(0, 8))
    if kind == "payload":
        img[at + FB.HEADER + int(rng.integers(0, k))] ^= bit
    elif kind == "crc":
        img[at + int(rng.integers(0, 4))] ^= bit
    elif kind == "length":  # past the block: by one byte, or by far
        left = FB.BLOCK - at % FB.BLOCK - FB.HEADER
        struct.pack_into("<H", img, at + 4, min(0xFFFF, left + 1) if rng.random() < 0.5 else 0xFFFF)
    else:  # a type out of range: with its checksum stale, or made good again (5 then ends the reading)
        img[at + 6] = int(rng.choice([0, 5, 6, 7, 200]))
        if rng.random() < 0.5:
            crc = oracle().extend(0, bytes(img[at + 6:at + FB.HEADER + k]))
            struct.pack_into("<I", img, at, mask1(crc))
            c.edges.add("type_with_good_checksum")
    c.edges.add("damage_" + kind)
    return len(img)


def gen_logread(c, rng):
    c.form = str(rng.choice(["log_walk", "log_read", "log_accept_gaps", "log_chains", "log_records"]))
    style = str(rng.choice(["tiny", "edge", "mixed", "long"]))
    n = draw_count(rng, {"tiny": MAX_ELEMENTS - 200, "edge": 300, "mixed": 200, "long": 20}[style])
    lens = draw_records(c, rng, n, style, 0)
    data = splitmix64_bytes(sum(lens) + 1, (c.seed * 1000003 + c.index) & U64, 0).tobytes()
    recs, q = [], 0
    for k in lens:
        recs.append(data[q:q + k])
        q += k
    img, phys = FB.log_image(recs, oracle())
    img, size, nd = bytearray(img), None, int(rng.choice([0, 0, 1, 2, 3, 5]))
    for kind in rng.choice(DAMAGES, nd):
        k = damage(c, rng, img, phys, str(kind))
        size = k if size is None else min(size, k)
    if nd >= 2:
        c.edges.add("two_damages")
    img = bytes(img[:size]) if size is not None else bytes(img)
    skew = int(rng.integers(0, 16))
    if skew:
        c.edges.add("skew")
    c.par.update(src_skew=skew, n=len(img))
    c.inp["src"] = np.frombuffer(bytes([0xEE]) * skew + img, np.uint8).copy()
    c.nbytes = len(img)
    nrec = sum(e[0] == "rec" for e in FB.log_scan(img))
    count_edges(c, nrec)
    kind = str(rng.choice(["below", "at", "above"]))
    cap = max(0, nrec + {"below": -1, "at": 0, "above": 3}[kind])
    c.edges.add("cap_" + kind)
    c.par["cap"] = cap
    c.elements = max(cap + 1, nrec)
    u64, u32, u8 = np.uint64, np.uint32, np.uint8
    walk = dict(off=(u64, cap), len=(u64, cap), stored=(u32, cap), type=(u8, cap), nrec=(u64, 1))
    verdict = dict(accept=(u8, cap), gap=(u8, cap), dropped=(u64, 1), bad_length=(u64, 1))
    chains = dict(first=(u64, cap + 1), whole=(u8, cap), frag_off=(u64, cap), frag_len=(u64, cap), nchain=(u64, 1),
                  nwhole=(u64, 1))
    if c.form == "log_walk":
        c.out.update(walk)
    elif c.form == "log_read":
        c.out.update(walk, ok=(u8, cap), **verdict)
    elif c.form == "log_accept_gaps":  # over the walk's arrays and verdicts of the caller's: some of them turned
        r = _log_read(c, cap)
        ok = r["ok"].copy()
        if cap and rng.random() < 0.7:
            ok ^= (rng.random(cap) < float(rng.choice([0.02, 0.3]))).astype(u8)
        c.inp.update(w_off=r["off"], w_len=r["len"], w_type=r["type"], w_ok=ok, w_nrec=r["nrec"])
        c.out.update(verdict)
    elif c.form == "log_chains":
        if rng.random() < 0.5:  # what the reader wrote for this image
            r = _log_read(c, cap)
            c.inp.update(w_type=r["type"], w_accept=r["accept"], w_gap=r["gap"], w_off=r["off"], w_len=r["len"],
                         w_nrec=r["nrec"])
        else:  # any triples: every type byte, gaps anywhere, a count above the arrays
            c.inp.update(w_type=rng.integers(0, 8, cap).astype(u8), w_accept=(rng.random(cap) < 0.85).astype(u8),
                         w_gap=(rng.random(cap) < 0.1).astype(u8), w_off=rng.integers(0, 1 << 40, cap).astype(u64),
                         w_len=rng.integers(0, 40000, cap).astype(u64),
                         w_nrec=np.array([[cap, cap + 5, cap // 2][int(rng.integers(0, 3))]], u64))
            c.edges.add("chains_random")
        if rng.random() < 0.3:
            del c.inp["w_gap"]
        c.out.update(chains)
    else:
        c.out.update(walk, ok=(u8, cap), rec_off=(u64, cap), rec_len=(u64, cap), end=(u64, 1), **verdict, **chains)
        draw_dst(c, rng, int(_log_records(c, cap)["end"][0]))
    c.desc = f"{style} records={n} damages={nd} n={len(img)} nrec={nrec} cap={cap} skew={skew}"


def gen_logwrite(c, rng):
    c.form = "log_frame"
    style = str(rng.choice(["tiny", "edge", "mixed", "long"]))
    n = draw_count(rng, {"tiny": MAX_ELEMENTS - 100, "edge": 300, "mixed": 200, "long": 20}[style])
    count_edges(c, n)
    dest_length = [0, FB.BLOCK, int(rng.integers(0, 1 << 40)),
                   5 * FB.BLOCK - int(rng.integers(0, 16))][int(rng.integers(0, 4))]
    lens = draw_records(c, rng, n, style, dest_length % FB.BLOCK)
    keep = (rng.random(n) < float(rng.choice([0.0, 0.5, 0.9, 1.01]))).astype(np.uint8) if rng.random() < 0.5 else None
    kept = np.ones(n, bool) if keep is None else keep != 0
    ln = np.array(lens, np.uint64).reshape(n)
    span = max(min(int(ln.sum()), 1 << 20), int(ln.max()) if n else 0, 64)
    pool(c, span)
    off = scatter(rng, ln, span)
    if keep is not None:  # a dropped record is never dereferenced: its off is KVSEP_OFFSET_SKIP, its length junk
        off[~kept] = np.uint64(SKIP)
        c.host["len"] = ln.copy()
        ln = ln.copy()
        ln[~kept] = np.uint64(0x7FFFFFFFFFFF)
        c.inp["keep"] = keep
        c.edges.add("keep_skip")
    phys, _, written = FB.writer([int(x) for x in c.host.get("len", ln)], kept, dest_length)
    nfrag = len(phys)
    kind = str(rng.choice(["below", "at", "above"]))
    frag_cap = max(0, nfrag + {"below": -1, "at": 0, "above": 3}[kind])
    c.edges.add("fragcap_" + kind)
    if nfrag and kind == "below":
        c.edges.add("refusal:frag_cut")
    if any(p[1] == FB.MIDDLE for p in phys):
        c.edges.add("many_fragments")
    draw_dst(c, rng, written)
    c.inp.update(off=off, len=ln)
    c.par.update(count=n, dest_length=dest_length, frag_cap=frag_cap, total=int(ln[kept].sum()) if n else 0)
    c.out.update(rec_at=(np.uint64, n), frag_first=(np.uint64, n + 1), frag_off=(np.uint64, frag_cap),
                 frag_len=(np.uint64, frag_cap), frag_at=(np.uint64, frag_cap), frag_type=(np.uint8, frag_cap),
                 frag_crc=(np.uint32, frag_cap), nfrag=(np.uint64, 1), written=(np.uint64, 1))
    c.elements = max(n, frag_cap)
    if rng.random() < 0.5:  # ... then the device reader over the bytes the device writer left
        c.form = "log_frame_records"
        rcap = nfrag + 3
        c.par["rcap"] = rcap
        c.elements = max(c.elements, rcap + 1)
        u64, u32, u8 = np.uint64, np.uint32, np.uint8
        for name, dt in (("off", u64), ("len", u64), ("stored", u32), ("type", u8), ("ok", u8), ("accept", u8),
                         ("gap", u8), ("whole", u8), ("frag_off", u64), ("frag_len", u64), ("rec_off", u64),
                         ("rec_len", u64)):
            c.out["r_" + name] = (dt, rcap)
        c.out["r_first"] = (u64, rcap + 1)
        for name in ("nrec", "dropped", "bad_length", "nchain", "nwhole", "end"):
            c.out["r_" + name] = (u64, 1)
        c.par["r_dst_bytes"] = int(ln[kept].sum()) + 64 if n else 64  # the kept payloads at most, and some room
        c.out["r_dst"] = (u8, c.par["r_dst_bytes"])
    c.desc = (f"{style} n={n} kept={int(kept.sum())} dest_length={dest_length} nfrag={nfrag} cap={frag_cap} "
              f"dst={c.par['dst_bytes']}/{written}")


def gen_sstread(c, rng):
    """Tables of sst_tables.build_table at restart interval 1, 2 or 16 with damage to data blocks, to the index block
    (the table form: the walk alone reads no checksum) or to the footer (the walk alone: an index handle that leaves the
    image), and a cap below, at and above what the table needs."""
    c.form = str(rng.choice(["sst_index", "sst_table_verify", "sst_index_keys"]))
    nblocks = draw_count(rng, 1100)
    count_edges(c, nblocks)
    interval = int(rng.choice([1, 2, 16]))
    c.edges.add(f"interval{interval}")
    img, off, ln, meta, index = T.build_table(nblocks, interval, seed=(c.seed * 1009 + c.index) % (1 << 31) + 1)
    n, table = img.size, c.form == "sst_table_verify"
    kind = str(rng.choice(["none", "data", "index", "footer"] if table else ["none", "data", "footer"]))
    handle = np.array(index, np.uint64)
    if kind == "data" and nblocks:
        for i in np.flatnonzero(bad_fraction(rng, nblocks)):
            img[int(off[i]) + int(rng.integers(0, int(ln[i]) + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        c.edges.add("damage_data")
    elif kind == "index":
        if rng.random() < 0.3:  # a type byte of 1 with the trailer a writer would give it
            blk = img[index[0]:index[0] + index[1]].tobytes()
            img[index[0] + index[1]:index[0] + index[1] + 5] = np.frombuffer(_trailer(blk, 1), np.uint8)
            c.edges.add("index_compressed")
        else:
            img[index[0] + int(rng.integers(0, index[1] + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
            c.edges.add("damage_index")
    elif kind == "footer":
        c.edges.add("refusal:bad_footer")
        if not table:  # off + len + 5 = n + 1, or far away
            handle = np.array([(index[0], n - index[0] - 4), (1 << 63, 1 << 63)][int(rng.integers(0, 2))], np.uint64)
        elif rng.random() < 0.3:
            n = int(rng.integers(0, 48))  # shorter than a footer
        else:
            img[n - 1 - int(rng.integers(0, 8))] ^= np.uint8(1 << int(rng.integers(0, 8)))  # a wrong magic
    if c.form == "sst_index_keys" and interval != 1 and nblocks > 1 and kind != "footer":
        c.edges.add("refusal:shared_key")
    skew = int(rng.integers(0, 16))
    if skew:
        c.edges.add("skew")
    c.inp["src"] = np.concatenate([np.full(skew, 0xEE, np.uint8), img])
    c.nbytes = img.size
    how = str(rng.choice(["below", "at", "above"]))
    c.edges.add("cap_" + how)
    need = nblocks + (2 if table else 0)
    cap = max(2 if table else 0, need + {"below": -1, "at": 0, "above": 3}[how])
    if c.host.get("member"):  # a sequence reserves nothing: the walk's scratch is sized by cap alone, so it holds the runs
        cap = max(cap, nblocks)
    c.par.update(src_skew=skew, n=n, cap=cap, reserve_count=max(cap, index[1] // 4 + 1), reserve=not c.host.get("member"))
    c.elements = max(nblocks, cap)
    u64, u32, u8 = np.uint64, np.uint32, np.uint8
    c.out.update(off=(u64, cap), len=(u64, cap), nblocks=(u64, 1), status=(u32, 1))
    if table:
        c.out.update(crc=(u32, cap), ok=(u8, cap), first_bad=(u64, 1), nbad=(u64, 1), bad_idx=(u64, cap),
                     handles=(u64, 4))
        c.par["max_len"] = draw_hint(rng, ln)
    else:
        c.inp["handle"] = handle
        if c.form == "sst_index_keys":
            c.out.update(key_off=(u64, cap), key_len=(u64, cap))
    c.desc = f"blocks={nblocks} interval={interval} damage={kind} n={n} cap={cap} skew={skew}"


VARINT_EDGES = [0, 1] + [v for b in range(7, 64, 7) for v in ((1 << b) - 1, 1 << b)] + [U64 - 1]


def gen_rewrite(c, rng):
    """A source table with damaged data blocks -- or one a rewrite refuses: restart interval 2, a bad footer, a damaged
    index block -- into a destination that is exact, one byte short or roomy."""
    nblocks = draw_count(rng, 1100)
    count_edges(c, nblocks)
    source = str(rng.choice(["good", "good", "good", "good", "interval2", "footer", "index"]))
    img, off, ln, meta, index = T.build_table(nblocks, 2 if source == "interval2" else 1,
                                              seed=(c.seed * 1013 + c.index) % (1 << 31) + 1)
    for i in np.flatnonzero(bad_fraction(rng, nblocks)):
        img[int(off[i]) + int(rng.integers(0, int(ln[i]) + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    if source == "footer":
        img[img.size - 1 - int(rng.integers(0, 8))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    elif source == "index":
        img[index[0] + int(rng.integers(0, index[1] + 5))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    skew = int(rng.integers(0, 16))
    if skew:
        c.edges.add("skew")
    c.inp["src"] = np.concatenate([np.full(skew, 0xEE, np.uint8), img])
    c.nbytes = img.size
    how = str(rng.choice(["below", "at", "above"]))
    cap = max(2, nblocks + 2 + {"below": -1, "at": 0, "above": 3}[how])
    if c.host.get("member"):
        cap = max(cap, nblocks)
    c.par.update(src_skew=skew, n=img.size, cap=cap, count=cap, max_len=draw_hint(rng, ln),
                 reserve_count=max(cap, index[1] // 4 + 1), reserve=not c.host.get("member"))
    c.elements = max(nblocks, cap)
    _, need, refuses = _rewrite(c, None)
    if refuses:
        c.edges.add("refusal:source")
    c.edges.add("rewrite_cap_" + how)
    draw_dst(c, rng, need, "no_room")
    u64, u32, u8 = np.uint64, np.uint32, np.uint8
    for name in ("off", "len", "key_off", "key_len", "dst_off"):
        c.out[name] = (u64, cap)
    c.out.update(crc=(u32, cap), ok=(u8, cap), handles=(u64, 4), status=(u32, 1), wstatus=(u32, 1))
    for name in ("nblocks", "nkept", "index_len", "table_bytes"):
        c.out[name] = (u64, 1)
    c.desc = f"blocks={nblocks} source={source} cap={cap} dst={c.par['dst_bytes']}/{need} skew={skew}"


def gen_sstwrite(c, rng):
    c.form = str(rng.choice(["sst_index_build", "sst_table_finish", "sst_table_rewrite"]))
    if c.form == "sst_table_rewrite":
        return gen_rewrite(c, rng)
    n = draw_count(rng)
    count_edges(c, n)
    style = str(rng.choice(["short", "mixed", "long"]))
    klen = rng.integers(0, 41, n).astype(np.uint64)
    if style != "short" and n:
        m = rng.random(n) < (0.03 if style == "mixed" else 0.3)
        klen[m] = rng.integers(100, 5001, int(m.sum())).astype(np.uint64)
        while int(klen.sum()) > MAX_PAYLOAD // 4:
            klen[klen > 100] //= np.uint64(2)
    span = max(1 << 16, int(klen.max()) if n else 0)
    pool(c, span)
    koff = scatter(rng, klen, span)
    pick = lambda: np.where(rng.random(n) < 0.5, np.array(VARINT_EDGES, np.uint64)[rng.integers(0, len(VARINT_EDGES), n)],  # noqa: E731
                            rng.integers(0, 1 << 62, n).astype(np.uint64) >> rng.integers(0, 62, n).astype(np.uint64))
    boff, blen = pick(), pick()
    if n and rng.random() < 0.5:
        boff[rng.random(n) < 0.2] = np.uint64(SKIP)  # what the salvage did not lay out
        c.edges.add("blk_skip")
    if rng.random() < 0.6:
        c.inp["keep"] = (rng.random(n) < float(rng.choice([0.0, 0.5, 0.95, 1.01]))).astype(np.uint8)
        c.edges.add("keep")
    kept = (boff != np.uint64(SKIP)) & (c.inp["keep"] != 0 if "keep" in c.inp else np.ones(n, bool))
    c.inp.update(key_off=koff, key_len=klen, blk_off=boff, blk_len=blen)
    c.par["count"] = n
    # a wavefront owns 64 consecutive entries and stages them when they encode to at most 4,096 bytes; a workgroup
    # owns 256: the edge is a workgroup with both kinds of wave
    size = np.array([3 + len(T.varint(int(klen[i]))) - 1 + int(klen[i]) + len(T.handle_bytes(int(boff[i]), int(blen[i])))
                     if kept[i] else 0 for i in range(n)], np.int64).reshape(n)
    for g0 in range(0, n, 256):
        waves = [int(size[w:w + 64].sum()) for w in range(g0, min(g0 + 256, n), 64)]
        if any(w > 4096 for w in waves) and any(0 < w <= 4096 for w in waves):
            c.edges.add("staged_and_unstaged")
        if sum(w > 4096 for w in waves) > 1:
            c.edges.add("several_unstaged")
    block = len(_index(c))
    at = int(rng.integers(0, 200))
    lead, trail = (13, 48) if c.form == "sst_table_finish" else (0, 0)
    draw_dst(c, rng, at + lead + block + 5 + trail, "no_room")
    c.inp["at"] = np.array([at], np.uint64)
    c.out.update(out_len=(np.uint64, 1), status=(np.uint32, 1))
    if c.form == "sst_table_finish":
        c.out["table_bytes"] = (np.uint64, 1)
    c.desc = (f"{style} n={n} kept={int(kept.sum())} block={block} at={at} dst={c.par['dst_bytes']} "
              f"skews={c.par['src_skew']}/{c.par['dst_skew']}")


# what each form asks of the scratch arrays it shares with other forms, in elements (include/kvsep_crc32c.h: the
# reserve notes of each entry point); only the sequence families' growth counter reads it
SCRATCH = {
    "verify_list": lambda c: {"list": c.par["count"] if c.par["bad_cap"] else 0},
    "sst_verify_list": lambda c: {"sst": c.par["count"], "list": c.par["count"] if c.par["bad_cap"] else 0},
    "concat": lambda c: {},
    "gather": lambda c: {},
    "pack": lambda c: {},
    "vlog_frame": lambda c: {},
    "vlog_frame_auto": lambda c: {"off": max(c.par["count"], c.par["nseg"])},
    "sst_frame": lambda c: {"sst": c.par["count"]},
    "offsets": lambda c: {"off": c.par["count"]},
    "salvage": lambda c: {"off": c.par["count"]},
    "sst_salvage": lambda c: {"sst": c.par["count"], "off": c.par["count"], "list": c.par["count"]},
    "log_walk": lambda c: {"log": -(-c.par["n"] // FB.BLOCK), "off": -(-c.par["n"] // FB.BLOCK)},
    "log_read": lambda c: {"log": -(-c.par["n"] // FB.BLOCK), "off": -(-c.par["n"] // FB.BLOCK)},
    "log_accept_gaps": lambda c: {"log": -(-c.par["n"] // FB.BLOCK)},
    "log_chains": lambda c: {"chain": c.par["cap"]},
    "log_records": lambda c: {"log": -(-c.par["n"] // FB.BLOCK), "chain": c.par["cap"], "off": c.par["cap"]},
    "log_frame": lambda c: {"logw": max(c.par["count"], c.par["frag_cap"])},
    "log_frame_records": lambda c: {"logw": max(c.par["count"], c.par["frag_cap"]), "chain": c.par["rcap"],
                                    "off": c.par["rcap"], "log": -(-c.par["dst_bytes"] // FB.BLOCK)},
    "sst_index": lambda c: {"sstidx": c.par["cap"], "off": c.par["cap"]},
    "sst_index_keys": lambda c: {"sstidx": c.par["cap"], "off": c.par["cap"]},
    "sst_table_verify": lambda c: {"sstidx": c.par["cap"], "off": c.par["cap"], "sst": c.par["cap"],
                                   "list": c.par["cap"]},
    "sst_table_rewrite": lambda c: {"sstidx": c.par["cap"], "off": c.par["cap"], "sst": c.par["cap"],
                                    "sstw": c.par["cap"]},
    "sst_index_build": lambda c: {"off": c.par["count"], "sstw": c.par["count"]},
    "sst_table_finish": lambda c: {"off": c.par["count"], "sstw": c.par["count"]},
}


def gen_sequence(c, rng):
    k = int(rng.integers(6, 11))
    fams = rng.choice(SINGLE, k)
    grown, held = {}, {}
    for j, f in enumerate(fams):
        m = make_case(str(f), c.seed, 100000 + 16 * c.index + j, member=True)  # the members' own (family, seed, index)
        c.members.append(m)
        c.elements += m.elements
        c.nbytes += m.nbytes
        for arr, need in SCRATCH[m.form](m).items():
            if need > held.get(arr, 0):
                held[arr] = need
                grown.setdefault(arr, set()).add(m.form)
    if c.family == "captured":  # and one call captured alone over a reservation one block short of it
        for j in range(8):
            m = make_case("layout", c.seed, 200000 + 16 * c.index + j, member=True)
            if m.form in ("offsets", "salvage") and m.par["count"] >= 2:
                c.refused = m
                c.edges.add("refusal:over_reservation")
                break
    if any(len(v) > 1 for v in grown.values()):
        c.edges.add("grown_by_two_forms")
    c.form = c.family
    c.desc = " ".join(m.form for m in c.members)


GENERATORS = {"lists": gen_lists, "combine": gen_combine, "frame": gen_frame, "layout": gen_layout,
              "logread": gen_logread, "sstread": gen_sstread, "logwrite": gen_logwrite, "sstwrite": gen_sstwrite, "sequence": gen_sequence, "captured": gen_sequence}


def make_case(family, seed, index, member=False):
    """member: the case runs inside a sequence, on a context that reserves nothing."""
    c = Case(family, seed, index)
    rng = np.random.default_rng([seed, FAMILY_ID[family], index])
    c.host.update(rng=rng, member=member)
    GENERATORS[family](c, rng)
    del c.host["rng"]
    assert c.elements <= MAX_ELEMENTS * (1 if not c.members else 16) and c.nbytes <= MAX_PAYLOAD * max(1, len(c.members))
    return c


# ========================================================================================================== models
def _base(c):
    return c.inp["src"][c.par["src_skew"]:]


def _canary_dst(c):
    return np.full(c.par["dst_bytes"], CANARY, np.uint8)


def _put(dst, at, data):
    """A range that does not lie inside the destination is not written at all."""
    if at + len(data) <= dst.size:
        dst[at:at + len(data)] = np.frombuffer(bytes(data), np.uint8)


def _list_outputs(c, crc, bad):
    n, cap = c.par["count"], c.par["bad_cap"]
    idx = np.flatnonzero(bad).astype(np.uint64)
    w = dict(out=crc, first_bad=np.array([idx[0] if idx.size else U64], np.uint64),
             nbad=np.array([idx.size], np.uint64))
    if "bad_idx" in c.out:
        w["bad_idx"] = np.full(cap, np.uint64(CANARY * 0x0101010101010101), np.uint64)  # past the list: as it was
        w["bad_idx"][:min(cap, idx.size)] = idx[:cap]
    if "ok" in c.out:
        w["ok"] = (~bad).astype(np.uint8).reshape(n)
    return w


def _sst_check(c):
    """table/format.cc:99-106 per handle: Value(block || type) against the unmasked stored word."""
    img, pos, ln = _base(c), c.inp["off"], c.inp["len"]
    crc = oracle().batch(img, pos, ln + np.uint64(1))
    stored = np.zeros(pos.size, np.uint32)
    for k in range(4):
        stored |= img[(pos + ln).astype(np.int64) + 1 + k].astype(np.uint32) << np.uint32(8 * k)
    return crc, mask32(crc) != stored


def model_verify_list(c):
    crc = oracle().batch(_base(c), c.inp["off"], c.inp["len"], c.inp.get("init"))
    return _list_outputs(c, crc, mask32(crc) != c.inp["expected"])


def model_sst_verify_list(c):
    return _list_outputs(c, *_sst_check(c))


def _runs(c):
    """Every first[] value clamped to nseg; a run that ends before it starts is empty."""
    first, nseg = c.inp["first"], c.par["nseg"]
    for i in range(c.par["count"]):
        yield i, range(min(int(first[i]), nseg), min(int(first[i + 1]), nseg))


def _segment(src, off, ln, j):
    return src[int(off[j]):int(off[j]) + int(ln[j])].tobytes()


def _combine(c, src, off):
    ln, init = c.inp["seg_len"], c.inp.get("init")
    out = np.zeros(c.par["count"], np.uint32)
    for i, run in _runs(c):
        out[i] = oracle().extend(0 if init is None else int(init[i]), b"".join(_segment(src, off, ln, j) for j in run))
    return out


def model_concat(c):
    return dict(out=_combine(c, c.host["src"], c.host["seg_off"]))


def model_gather(c):
    return dict(out=_combine(c, _base(c), c.inp["seg_off"]),
                seg_crc=oracle().batch(_base(c), c.inp["seg_off"], c.inp["seg_len"]))


def _payloads(c):
    src, off, ln = _base(c), c.inp["seg_off"], c.inp["seg_len"]
    return [b"".join(_segment(src, off, ln, j) for j in run) for _, run in _runs(c)]


def model_pack(c):
    dst = _canary_dst(c)
    for p, at in zip(_payloads(c), c.inp["dst_off"]):
        _put(dst, int(at), p)
    return dict(dst=dst)


def _vlog(c, at):
    """db/value_log_writer.cc:46-76: [Mask(Value(p)) LE32][len LE32][p]."""
    dst, pay = _canary_dst(c), _payloads(c)
    crc = np.array([oracle().extend(0, p) for p in pay], np.uint32).reshape(len(pay))
    for p, v, a in zip(pay, crc, at):
        _put(dst, int(a), struct.pack("<II", mask1(v), len(p) & 0xFFFFFFFF) + p)
    return dict(dst=dst, crc_out=crc, seg_crc=oracle().batch(_base(c), c.inp["seg_off"], c.inp["seg_len"]))


def model_vlog_frame(c):
    return _vlog(c, c.inp["dst_off"])


def model_vlog_frame_auto(c):
    at, p = [], c.par["start"]
    for pay in _payloads(c):
        at.append(p)
        p += 8 + len(pay)
    w = _vlog(c, at)
    w.update(rec_off=np.array(at, np.uint64).reshape(len(at)), end=np.array([p], np.uint64))
    return w


def model_sst_frame(c):
    """table/table_builder.cc:209-232: [block][type][Mask(Extend(Value(block), type)) LE32]."""
    dst, src = _canary_dst(c), _base(c)
    words = np.zeros(c.par["count"], np.uint32)
    for i in range(c.par["count"]):
        blk, t = _segment(src, c.inp["off"], c.inp["len"], i), bytes([int(c.inp["types"][i])])
        words[i] = mask1(oracle().extend(oracle().extend(0, blk), t))
        _put(dst, int(c.inp["blk_off"][i]), blk + t + struct.pack("<I", int(words[i])))
    return dict(dst=dst, masked_out=words)


def _offsets(c, seg_len, first, keep, head, tail, start):
    before = int(c.inp["keep_before"][0]) if "keep_before" in c.inp else None
    dst_off, end, nk, _ = FB.ref_offsets(seg_len, first, keep, before, head, tail, start, U64, c.par["count"])
    return dict(dst_off=dst_off.reshape(c.par["count"]), end=np.array([end], np.uint64),
                nkept=np.array([nk], np.uint64))


def model_offsets(c):
    return _offsets(c, c.inp["seg_len"], c.inp.get("first"), c.inp.get("keep"), c.par["head"], c.par["tail"],
                    c.par["start"])


def _salvage(c, w, extra):
    dst, src = _canary_dst(c), _base(c)
    for i, at in enumerate(w["dst_off"]):
        if int(at) != SKIP:
            o = int(c.inp["off"][i])
            _put(dst, int(at), src[o:o + int(c.inp["len"][i]) + extra].tobytes())
    w["dst"] = dst
    return w


def model_salvage(c):
    return _salvage(c, _offsets(c, c.inp["len"], None, c.inp.get("keep"), 0, 0, 0), 0)


def model_sst_salvage(c):
    crc, bad = _sst_check(c)
    c2 = copy.copy(c)
    c2.par = dict(c.par, bad_cap=0)
    w = _list_outputs(c2, crc, bad)
    w.update(_offsets(c, c.inp["len"], None, (~bad).astype(np.uint8), 0, 5, 0))
    return _salvage(c, w, 5)


def _log_read(c, cap, img=None, ok=None):
    """log::Reader's physical records and verdicts for the first min(nrec, cap) of them, padded to cap."""
    img = bytes(_base(c)[:c.par["n"]]) if img is None else img
    ev = FB.log_scan(img)
    recs = [e for e in ev if e[0] == "rec"]
    cnt = min(len(recs), cap)
    off, ln, st, ty = (np.zeros(cap, d) for d in (np.uint64, np.uint64, np.uint32, np.uint8))
    for i, (_, p, k, t, w) in enumerate(recs[:cnt]):
        off[i], ln[i], st[i], ty[i] = p + 6, 1 + k, w, t
    if ok is None:
        ok = np.zeros(cap, np.uint8)
        ok[:cnt] = mask32(oracle().batch(np.frombuffer(img + b"\0", np.uint8), off[:cnt], ln[:cnt])) == st[:cnt]
    accept, gap, dropped, bad = FB.log_accept(ev, len(img), ok, cnt)
    pad = [0] * (cap - cnt)
    return dict(off=off, len=ln, stored=st, type=ty, ok=ok, nrec=np.array([len(recs)], np.uint64),
                accept=np.array(accept + pad, np.uint8).reshape(cap), gap=np.array(gap + pad, np.uint8).reshape(cap),
                dropped=np.array([dropped], np.uint64), bad_length=np.array([bad], np.uint64))


def _log_chains(cap, nrec, ty, accept, gap, off, ln):
    cnt = min(int(nrec), cap)
    first, whole, nchain = FB.log_chain_table(ty[:cnt], accept[:cnt], gap[:cnt])
    fo, fl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    for i in range(cnt):
        fo[i], fl[i] = int(off[i]) + 1, max(int(ln[i]) - 1, 0)
    return dict(first=np.array(first + [cnt] * (cap - cnt), np.uint64).reshape(cap + 1),
                whole=np.array(whole + [0] * (cap - cnt), np.uint8).reshape(cap), frag_off=fo, frag_len=fl,
                nchain=np.array([nchain], np.uint64), nwhole=np.array([sum(whole)], np.uint64))


def _log_records(c, cap, img=None, dst_bytes=None):
    """The records log::Reader returns, back to back (db/log_reader.cc:58-173)."""
    img = bytes(_base(c)[:c.par["n"]]) if img is None else img
    w = _log_read(c, cap, img)
    w.update(_log_chains(cap, w["nrec"][0], w["type"], w["accept"], w["gap"], w["off"], w["len"]))
    dst_bytes = c.par.get("dst_bytes") if dst_bytes is None else dst_bytes
    dst = None if dst_bytes is None else np.full(dst_bytes, CANARY, np.uint8)  # None: only the bytes needed are asked
    rec_off, rec_len, pos = np.full(cap, SKIP, np.uint64), np.zeros(cap, np.uint64), 0
    for j in range(int(w["nchain"][0])):
        if w["whole"][j]:
            data = b"".join(img[int(w["frag_off"][i]):int(w["frag_off"][i]) + int(w["frag_len"][i])]
                            for i in range(int(w["first"][j]), int(w["first"][j + 1])))
            rec_off[j], rec_len[j] = pos, len(data)
            if dst is not None:
                _put(dst, pos, data)
            pos += len(data)
    w.update(rec_off=rec_off, rec_len=rec_len, end=np.array([pos], np.uint64))
    if dst is not None:
        w["dst"] = dst
    return w


def _only(c, w):
    return {k: v for k, v in w.items() if k in c.out}


def model_log_walk(c):
    return _only(c, _log_read(c, c.par["cap"]))


def model_log_read(c):
    return _only(c, _log_read(c, c.par["cap"]))


def model_log_accept_gaps(c):
    return _only(c, _log_read(c, c.par["cap"], ok=c.inp["w_ok"]))


def model_log_chains(c):
    cap = c.par["cap"]
    return _log_chains(cap, c.inp["w_nrec"][0], c.inp["w_type"], c.inp["w_accept"],
                       c.inp["w_gap"] if "w_gap" in c.inp else np.zeros(cap, np.uint8), c.inp["w_off"], c.inp["w_len"])


def model_log_records(c):
    return _only(c, _log_records(c, c.par["cap"]))


def model_log_frame(c):
    """log::Writer::AddRecord and EmitPhysicalRecord (db/log_writer.cc:35-115) for the kept records."""
    n, cap, src = c.par["count"], c.par["frag_cap"], _base(c)
    keep = c.inp["keep"] if "keep" in c.inp else np.ones(n, np.uint8)
    lens = [int(x) for x in c.host.get("len", c.inp["len"])]
    phys, pads, written = FB.writer(lens, keep, c.par["dest_length"])
    rec_at, first = np.full(n, SKIP, np.uint64), np.zeros(n + 1, np.uint64)
    fo, fl, ft = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    fa, fc = np.full(cap, SKIP, np.uint64), np.zeros(cap, np.uint32)
    dst = _canary_dst(c)
    for f, (at, t, k, r, rpos) in enumerate(phys):
        if rpos == 0 and (t in (FB.FULL, FB.FIRST)):
            rec_at[r] = at
        first[r + 1:] = f + 1
        if f >= cap:
            continue
        o = int(c.inp["off"][r]) + rpos
        data = src[o:o + k].tobytes()
        crc = oracle().extend(oracle().extend(0, bytes([t])), data)
        fo[f], fl[f], fa[f], ft[f], fc[f] = o, k, at, t, crc
        _put(dst, at, struct.pack("<IHB", mask1(crc), k, t) + data)
    for at, k, r in pads:  # the zero trailer goes with the record behind it
        if int(first[r]) < cap:
            _put(dst, at, bytes(k))
    return dict(rec_at=rec_at, frag_first=first, frag_off=fo, frag_len=fl, frag_at=fa, frag_type=ft, frag_crc=fc,
                nfrag=np.array([len(phys)], np.uint64), written=np.array([written], np.uint64), dst=dst)


def _usable(off, ln, n):
    """A handle whose block and 5-byte trailer lie inside the image."""
    return off + ln + 5 <= n


def _footer(img):
    """Footer::DecodeFrom (table/format.cc:37-60) -> (meta_off, meta_len, index_off, index_len) or None."""
    n = len(img)
    if n < 48 or int.from_bytes(img[n - 8:], "little") != T.MAGIC:
        return None
    h, p = [], n - 48
    try:
        for _ in range(4):
            v, p = T.get_varint(img, p, n - 8)
            h.append(v)
    except ValueError:
        return None
    return tuple(h) if _usable(h[0], h[1], n) and _usable(h[2], h[3], n) else None


def _entries(block, base):
    """Block::Iter over an intact index block -> [(shared, key offset in the image, unshared key bytes, off, len)]."""
    n = len(block)
    ro = n - 4 * (1 + int.from_bytes(block[n - 4:], "little"))
    out, p = [], 0
    while p < ro:
        shared, p = T.get_varint(block, p, ro, 5)
        non_shared, p = T.get_varint(block, p, ro, 5)
        vlen, p = T.get_varint(block, p, ro, 5)
        v = p + non_shared
        off, q = T.get_varint(block, v, v + vlen)
        ln, q = T.get_varint(block, q, v + vlen)
        out.append((shared, base + p, non_shared, off, ln))
        p = v + vlen
    return out


def _read_check(img, off, ln):
    """table/format.cc:99-106 for one block -> (Value(block || type), passes)."""
    crc = oracle().extend(0, img[off:off + ln + 1])
    return crc, mask1(crc) == int.from_bytes(img[off + ln + 1:off + ln + 5], "little")


def _sst_walk(c, keys):
    cap, img = c.par["cap"], _base(c)[:c.par["n"]].tobytes()
    ioff, ilen = (int(x) for x in c.inp["handle"])
    w = {k: np.zeros(cap, np.uint64) for k in ("off", "len", "key_off", "key_len")}
    status, ent = SST_OK, []
    if not _usable(ioff, ilen, len(img)):
        status = SST_BAD_FOOTER
    else:
        for e in _entries(img[ioff:ioff + ilen], ioff):
            if keys and e[0]:  # a key that shares bytes has no contiguous place: the walk stops in front of it
                status = SST_SHARED_KEY
                break
            ent.append(e)
    for i, e in enumerate(ent[:cap]):
        w["key_off"][i], w["key_len"][i], w["off"][i], w["len"][i] = e[1:]
    w.update(nblocks=np.array([len(ent)], np.uint64), status=np.array([status], np.uint32))
    return _only(c, w)


def model_sst_index(c):
    return _sst_walk(c, False)


def model_sst_index_keys(c):
    return _sst_walk(c, True)


def _sst_table(c, keys=False):
    """The table form's slots and verdicts -> (outputs, the data slots' number, the source refuses a rewrite)."""
    cap, img = c.par["cap"], _base(c)[:c.par["n"]].tobytes()
    off, ln, crc, ok = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.ones(cap, np.uint8)
    koff, klen = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    h, status, nblocks, slots, ent = _footer(img), SST_OK, 0, [], []
    if h is None:
        status, h = SST_BAD_FOOTER, (0, 0, 0, 0)
    else:
        _, good = _read_check(img, h[2], h[3])
        if not good:
            status = SST_INDEX_CHECKSUM
        elif img[h[2] + h[3]] != 0:
            status = SST_INDEX_COMPRESSED
        else:
            for e in _entries(img[h[2]:h[2] + h[3]], h[2]):
                if keys and e[0]:
                    status = SST_SHARED_KEY
                    break
                ent.append(e)
            nblocks = len(ent)
            if status == SST_OK and nblocks + 2 > cap:
                status = SST_CAP
            ent = ent[:min(nblocks, cap - 2)]
            slots = [e[3:] for e in ent]
        slots = slots + [h[:2], h[2:]]
    for i, e in enumerate(ent):
        koff[i], klen[i] = e[1], e[2]
    for i, (o, k) in enumerate(slots):
        off[i], ln[i] = o, k
        if _usable(o, k, len(img)):
            crc[i], good = _read_check(img, o, k)
            ok[i] = int(good)
        else:  # reported bad, never dereferenced
            ok[i] = 0
    w = dict(off=off, len=ln, crc=crc, ok=ok, key_off=koff, key_len=klen, handles=np.array(h, np.uint64),
             nblocks=np.array([nblocks], np.uint64), status=np.array([status], np.uint32))
    return w, len(ent), status in (SST_BAD_FOOTER, SST_INDEX_CHECKSUM, SST_INDEX_COMPRESSED, SST_SHARED_KEY)


def model_sst_table_verify(c):
    w, _, _ = _sst_table(c)
    c2 = copy.copy(c)
    c2.par = dict(c.par, count=c.par["cap"], bad_cap=c.par["cap"])
    lists = _list_outputs(c2, w["crc"], w["ok"] == 0)
    del lists["out"], w["key_off"], w["key_len"]
    w.update(lists)
    return w


def _rewrite(c, dst_bytes):
    """The source without its bad blocks, as a table: the kept blocks with their trailers back to back, the empty
    metaindex block, BlockBuilder's index block over the kept keys and the new handles, the footer."""
    cap, img = c.par["cap"], _base(c)[:c.par["n"]].tobytes()
    w, m, refuses = _sst_table(c, keys=True)
    keep = np.zeros(cap, np.uint8)
    if not refuses:
        keep[:m] = w["ok"][:m]
    dst_off, data_end, nkept, _ = FB.ref_offsets(w["len"], None, keep, None, 0, 5, 0, U64, cap)
    dst = np.full(dst_bytes if dst_bytes is not None else 0, CANARY, np.uint8)
    keys, handles = [], []
    for i in np.flatnonzero(keep):
        o, k = int(w["off"][i]), int(w["len"][i])
        if dst_bytes is not None:
            _put(dst, int(dst_off[i]), img[o:o + k + 5])
        keys.append(img[int(w["key_off"][i]):int(w["key_off"][i]) + int(w["key_len"][i])])
        handles.append((int(dst_off[i]), k))
    index_len = table_bytes = 0
    wstatus, need = 3, len(img)  # KVSEP_SSTW_SOURCE: there is no index to rewrite
    if not refuses:
        meta, idx = T.index_block([], [], 1), T.index_block(keys, handles, 1)
        table = meta + _trailer(meta) + idx + _trailer(idx) + T.footer((data_end, 8), (data_end + 13, len(idx)))
        index_len, need = len(idx), data_end + len(table)
        wstatus = SSTW_OK if dst_bytes is None or need <= dst_bytes else SSTW_NO_ROOM
        if dst_bytes is not None and wstatus == SSTW_OK:
            _put(dst, data_end, table)
            table_bytes = need
    w.update(dst_off=dst_off.reshape(cap), nkept=np.array([nkept], np.uint64), dst=dst,
             index_len=np.array([index_len], np.uint64), table_bytes=np.array([table_bytes], np.uint64),
             wstatus=np.array([wstatus], np.uint32))
    return w, need, refuses


def model_sst_table_rewrite(c):
    return _rewrite(c, c.par["dst_bytes"])[0]


def model_log_frame_records(c):
    """The frame form's outputs, and what log::Reader makes of the destination as the call must leave it."""
    frame_out = {k: v for k, v in c.out.items() if not k.startswith("r_")}
    c1 = copy.copy(c)
    c1.out = frame_out
    w = model_log_frame(c1)
    r = _log_records(c, c.par["rcap"], img=w["dst"].tobytes(), dst_bytes=c.par["r_dst_bytes"])
    w.update({"r_" + k: v for k, v in r.items()})
    return w


def _trailer(block, type_byte=0):
    t = bytes([type_byte])
    return t + struct.pack("<I", mask1(oracle().extend(oracle().extend(0, block), t)))


def _index(c):
    """BlockBuilder at restart interval 1 over the kept entries (tests/sst_tables.index_block)."""
    src, n = _base(c), c.par["count"]
    keep = c.inp["keep"] if "keep" in c.inp else np.ones(n, np.uint8)
    keys, handles = [], []
    for i in range(n):
        if keep[i] and int(c.inp["blk_off"][i]) != SKIP:
            keys.append(_segment(src, c.inp["key_off"], c.inp["key_len"], i))
            handles.append((int(c.inp["blk_off"][i]), int(c.inp["blk_len"][i])))
    return T.index_block(keys, handles, 1)


def model_sst_index_build(c):
    dst, blk, at = _canary_dst(c), _index(c), int(c.inp["at"][0])
    fits = at + len(blk) + 5 <= dst.size
    if fits:
        _put(dst, at, blk + _trailer(blk))
    return dict(dst=dst, out_len=np.array([len(blk)], np.uint64),
                status=np.array([SSTW_OK if fits else SSTW_NO_ROOM], np.uint32))


def model_sst_table_finish(c):
    dst, blk, at = _canary_dst(c), _index(c), int(c.inp["at"][0])
    meta = T.index_block([], [], 1)
    table = meta + _trailer(meta) + blk + _trailer(blk) + T.footer((at, len(meta)), (at + 13, len(blk)))
    fits = at + len(table) <= dst.size
    if fits:
        _put(dst, at, table)
    return dict(dst=dst, out_len=np.array([len(blk)], np.uint64),
                table_bytes=np.array([at + len(table) if fits else 0], np.uint64),
                status=np.array([SSTW_OK if fits else SSTW_NO_ROOM], np.uint32))


MODELS = {k[6:]: v for k, v in list(globals().items()) if k.startswith("model_")}


def expect(c):
    """Every output array and destination byte of the case's call -> {name: array}; a sequence: one per member."""
    if c.members:
        return [expect(m) for m in c.members]
    w = MODELS[c.form](c)
    assert set(w) == set(c.out), (c.form, sorted(w), sorted(c.out))
    return w


# ====================================================================================================== comparator
def sentinel(dtype):
    return np.frombuffer(bytes([CANARY]) * 8, np.uint8).view(dtype)[0]


def is_dst(name):
    return name.endswith("dst")


def guard_lo(c, name):
    return c.par.get(name + "_skew", 0) + DG if is_dst(name) else G


def as_got(c, want):
    """What the runner would return for a device that wrote exactly `want`: the arrays between their guards and the
    inputs as they went in.  The CPU tests feed compare() through this."""
    got = {}
    for name, w in want.items():
        dtype, n = c.out[name]
        w = np.asarray(w, dtype).reshape(n)
        if is_dst(name):
            raw = np.full(SKEW + 2 * DG + n, CANARY, np.uint8)
        else:
            raw = np.full(n + 2 * G, sentinel(dtype), dtype)
        lo = guard_lo(c, name)
        raw[lo:lo + n] = w
        got[name] = raw
    for name, a in c.inp.items():
        got["in:" + name] = a.copy()
    return got


def compare(c, got, want, only=None):
    """Every output element, the guards, the inputs; raises Mismatch naming the first difference."""
    def fail(name, index, g, w):
        raise Mismatch(f"{c.line()}: {name}[{index}] = {g} want {w}", name, index)

    for name in sorted(want):
        if only is not None and name not in only:
            continue
        dtype, n = c.out[name]
        w = np.asarray(want[name], dtype).reshape(n)
        raw, lo = got[name], guard_lo(c, name)
        if raw.dtype != dtype or raw.size < lo + n:
            raise Mismatch(f"{c.line()}: {name}: {raw.dtype}[{raw.size}] returned for {dtype}[{n}]", name, None)
        d = np.flatnonzero(raw[lo:lo + n] != w)
        if d.size:
            fail(name, int(d[0]), raw[lo + d[0]], w[d[0]])
        s = CANARY if is_dst(name) else sentinel(dtype)
        d = np.flatnonzero(raw != s)
        d = d[(d < lo) | (d >= lo + n)]
        if d.size:  # an index below 0 or at / past n: a guard element
            fail(name, int(d[0]) - lo, raw[d[0]], s)
    if only is None:
        for name, a in c.inp.items():
            d = np.flatnonzero(got["in:" + name] != a)
            if d.size:
                fail("in:" + name, int(d[0]), got["in:" + name][d[0]], a[d[0]])


# ========================================================================================================== runner
class Device:
    """One case's arrays on the device: the inputs as they are, every output between guards, all canary-filled."""

    def __init__(self, c):
        import torch
        self.c, self.torch, self.dev = c, torch, torch.device("cuda:0")
        self.inp, self.out = {}, {}
        for name, a in c.inp.items():
            self.inp[name] = self._upload(a)
        for name, (dtype, n) in c.out.items():
            nbytes = SKEW + 2 * DG + n if is_dst(name) else (n + 2 * G) * np.dtype(dtype).itemsize
            self.out[name] = torch.full((nbytes,), CANARY, dtype=torch.uint8, device=self.dev)

    def _upload(self, a):
        raw = np.zeros(a.nbytes + 16, np.uint8)  # never an empty allocation: a null pointer means "absent"
        raw[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return self.torch.from_numpy(raw).to(self.dev)

    def rewrite(self, c):
        """The inputs of another case of the same shapes, in place."""
        self.c = c
        for name, a in c.inp.items():
            self.inp[name][:a.nbytes] = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
        for t in self.out.values():
            t.fill_(CANARY)

    def i(self, name):
        if name not in self.inp:
            return None
        return self.inp[name].data_ptr() + (self.c.par["src_skew"] if name == "src" else 0)

    def o(self, name):
        if name not in self.out:
            return None
        dtype = self.c.out[name][0]
        return self.out[name].data_ptr() + guard_lo(self.c, name) * np.dtype(dtype).itemsize

    def download(self):
        got = {}
        for name, t in self.out.items():
            got[name] = t.cpu().numpy().view(self.c.out[name][0])
        for name, a in self.c.inp.items():
            got["in:" + name] = self.inp[name].cpu().numpy()[:a.nbytes].view(a.dtype).reshape(a.shape)
        return got


def call(ctx, d, s):
    """The device call of d's case, asynchronous on stream s."""
    c, i, o, p = d.c, d.i, d.o, d.c.par
    f = c.form
    if f == "verify_list":
        ctx.verify_list_device(i("src"), i("off"), i("len"), i("expected"), o("out"), o("first_bad"), o("nbad"),
                               bad_idx=o("bad_idx"), bad_cap=p["bad_cap"], ok=o("ok"), init=i("init"),
                               count=p["count"], total_bytes=p["total"], max_len=p["max_len"], stream=s)
    elif f == "sst_verify_list":
        ctx.sst_verify_list_device(i("src"), i("off"), i("len"), o("out"), o("first_bad"), o("nbad"),
                                   bad_idx=o("bad_idx"), bad_cap=p["bad_cap"], ok=o("ok"), count=p["count"],
                                   total_bytes=p["total"], max_len=p["max_len"], stream=s)
    elif f == "concat":
        ctx.concat_device(i("seg_crc"), i("seg_len"), i("first"), o("out"), init=i("init"), count=p["count"],
                          nseg=p["nseg"], stream=s)
    elif f == "gather":
        ctx.gather_device(i("src"), i("seg_off"), i("seg_len"), i("first"), o("seg_crc"), o("out"), init=i("init"),
                          count=p["count"], nseg=p["nseg"], total_bytes=p["total"], max_len=p["max_len"], stream=s)
    elif f == "pack":
        ctx.pack_device(i("src"), i("seg_off"), i("seg_len"), i("first"), o("dst"), p["dst_bytes"], i("dst_off"),
                        count=p["count"], nseg=p["nseg"], stream=s)
    elif f == "vlog_frame":
        ctx.vlog_frame_device(i("src"), i("seg_off"), i("seg_len"), i("first"), o("seg_crc"), o("crc_out"), o("dst"),
                              p["dst_bytes"], i("dst_off"), count=p["count"], nseg=p["nseg"], total_bytes=p["total"],
                              max_len=p["max_len"], stream=s)
    elif f == "vlog_frame_auto":
        ctx.vlog_frame_auto_device(i("src"), i("seg_off"), i("seg_len"), i("first"), o("seg_crc"), o("crc_out"),
                                   o("dst"), p["dst_bytes"], o("rec_off"), o("end"), start=p["start"],
                                   count=p["count"], nseg=p["nseg"], total_bytes=p["total"], max_len=p["max_len"],
                                   stream=s)
    elif f == "sst_frame":
        ctx.sst_frame_device(i("src"), i("off"), i("len"), i("types"), o("masked_out"), o("dst"), p["dst_bytes"],
                             i("blk_off"), count=p["count"], total_bytes=p["total"], max_len=p["max_len"], stream=s)
    elif f == "offsets":
        ctx.offsets_device(i("seg_len"), o("dst_off"), o("end"), first=i("first"), keep=i("keep"),
                           keep_before=i("keep_before"), head=p["head"], tail=p["tail"], start=p["start"],
                           nkept=o("nkept"), count=p["count"], nseg=p["nseg"], stream=s)
    elif f == "salvage":
        ctx.salvage_device(i("src"), i("off"), i("len"), o("dst"), p["dst_bytes"], o("dst_off"), o("end"),
                           keep=i("keep"), keep_before=i("keep_before"), nkept=o("nkept"), count=p["count"], stream=s)
    elif f == "sst_salvage":
        ctx.sst_salvage_device(i("src"), i("off"), i("len"), o("out"), o("ok"), o("dst"), p["dst_bytes"], o("dst_off"),
                               o("end"), first_bad=o("first_bad"), nbad=o("nbad"), nkept=o("nkept"), count=p["count"],
                               total_bytes=p["total"], max_len=p["max_len"], stream=s)
    elif f == "log_walk":
        ctx.log_walk_device(i("src"), p["n"], o("nrec"), off=o("off"), length=o("len"), stored=o("stored"),
                            type=o("type"), cap=p["cap"], stream=s)
    elif f == "log_read":
        ctx.log_read_device(i("src"), p["n"], o("off"), o("len"), o("stored"), o("type"), o("ok"), o("accept"),
                            o("nrec"), gap=o("gap"), dropped=o("dropped"), bad_length=o("bad_length"), cap=p["cap"],
                            stream=s)
    elif f == "log_accept_gaps":
        ctx.log_accept_gaps_device(i("src"), p["n"], i("w_off"), i("w_len"), i("w_type"), i("w_ok"), i("w_nrec"),
                                   o("accept"), gap=o("gap"), dropped=o("dropped"), bad_length=o("bad_length"),
                                   cap=p["cap"], stream=s)
    elif f == "log_chains":
        ctx.log_chains_device(i("w_type"), i("w_accept"), i("w_nrec"), o("first"), o("whole"), o("nchain"),
                              gap=i("w_gap"), off=i("w_off"), length=i("w_len"), frag_off=o("frag_off"),
                              frag_len=o("frag_len"), nwhole=o("nwhole"), cap=p["cap"], stream=s)
    elif f == "log_records":
        ctx.log_records_device(i("src"), p["n"], o("off"), o("len"), o("stored"), o("type"), o("ok"), o("accept"),
                               o("gap"), o("nrec"), o("frag_off"), o("frag_len"), o("first"), o("whole"), o("nchain"),
                               o("dst"), p["dst_bytes"], o("rec_off"), o("end"), rec_len=o("rec_len"),
                               nwhole=o("nwhole"), dropped=o("dropped"), bad_length=o("bad_length"), cap=p["cap"],
                               stream=s)
    elif f in ("log_frame", "log_frame_records"):
        ctx.log_frame_device(i("src"), i("off"), i("len"), p["dest_length"], o("dst"), p["dst_bytes"], o("rec_at"),
                             o("frag_first"), o("frag_off"), o("frag_len"), o("frag_at"), o("frag_type"),
                             o("frag_crc"), o("nfrag"), o("written"), keep=i("keep"), count=p["count"],
                             frag_cap=p["frag_cap"], total_bytes=p["total"], stream=s)
        if f == "log_frame_records":
            ctx.log_records_device(o("dst"), p["dst_bytes"], o("r_off"), o("r_len"), o("r_stored"), o("r_type"),
                                   o("r_ok"), o("r_accept"), o("r_gap"), o("r_nrec"), o("r_frag_off"),
                                   o("r_frag_len"), o("r_first"), o("r_whole"), o("r_nchain"), o("r_dst"),
                                   p["r_dst_bytes"], o("r_rec_off"), o("r_end"), rec_len=o("r_rec_len"),
                                   nwhole=o("r_nwhole"), dropped=o("r_dropped"), bad_length=o("r_bad_length"),
                                   cap=p["rcap"], stream=s)
    elif f in ("sst_index", "sst_index_keys", "sst_table_verify"):
        if p["reserve"]:  # the sizing the header prescribes: the restart count is device data
            ctx.reserve(p["reserve_count"], p["n"] + 64)
        if f == "sst_index":
            ctx.sst_index_device(i("src"), p["n"], i("handle"), o("off"), o("len"), o("nblocks"), o("status"),
                                 cap=p["cap"], stream=s)
        elif f == "sst_index_keys":
            ctx.sst_index_keys_device(i("src"), p["n"], i("handle"), o("off"), o("len"), o("key_off"), o("key_len"),
                                      o("nblocks"), o("status"), cap=p["cap"], stream=s)
        else:
            ctx.sst_table_verify_device(i("src"), p["n"], o("off"), o("len"), o("crc"), o("ok"), o("nblocks"),
                                        o("handles"), o("status"), first_bad=o("first_bad"), nbad=o("nbad"),
                                        bad_idx=o("bad_idx"), bad_cap=p["cap"], cap=p["cap"],
                                        max_len_hint=p["max_len"], stream=s)
    elif f == "sst_table_rewrite":
        if p["reserve"]:
            ctx.reserve(p["reserve_count"], 2 * p["n"] + p["dst_bytes"] + p["cap"] + 64)
        ctx.sst_table_rewrite_device(i("src"), p["n"], o("dst"), p["dst_bytes"], o("off"), o("len"), o("key_off"),
                                     o("key_len"), o("crc"), o("ok"), o("dst_off"), o("nblocks"), o("handles"),
                                     o("status"), o("index_len"), o("table_bytes"), o("wstatus"), nkept=o("nkept"),
                                     cap=p["cap"], max_len_hint=p["max_len"], stream=s)
    elif f == "sst_index_build":
        ctx.sst_index_build_device(i("src"), i("key_off"), i("key_len"), i("blk_off"), i("blk_len"), o("dst"),
                                   p["dst_bytes"], i("at"), o("out_len"), o("status"), keep=i("keep"),
                                   count=p["count"], stream=s)
    elif f == "sst_table_finish":
        ctx.sst_table_finish_device(i("src"), i("key_off"), i("key_len"), i("blk_off"), i("blk_len"), o("dst"),
                                    p["dst_bytes"], i("at"), o("out_len"), o("table_bytes"), o("status"),
                                    keep=i("keep"), count=p["count"], stream=s)
    else:
        raise KeyError(f)


def run_case(ctx, c, stream=None):
    """Upload, call, download -> what compare() takes.  The sequence families make their own fresh context: the mixed
    calls of `sequence` alternate between two streams with no host step between them and are read after one final
    synchronise; `captured` reserves for its largest member, captures every call into one graph on one stream and
    replays it twice, the second time over inputs rewritten in place."""
    import torch
    if not c.members:
        d = Device(c)
        torch.cuda.synchronize()
        call(ctx, d, stream if stream is not None else torch.cuda.current_stream())
        torch.cuda.synchronize()
        return d.download()
    import kvsep
    own = kvsep.Context(0)
    try:
        ds = [Device(m) for m in c.members]
        torch.cuda.synchronize()
        if c.family == "sequence":
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for j, d in enumerate(ds):
                call(own, d, streams[j % 2])
            torch.cuda.synchronize()
            return [d.download() for d in ds]
        own.reserve(max(max(max(m.elements, m.par.get("reserve_count", 0)) for m in c.members), 1),
                    max(max(m.nbytes, m.par.get("total", 0), m.par.get("dst_bytes", 0)) for m in c.members) + (1 << 20))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for d in ds:
                call(own, d, torch.cuda.current_stream())
        g.replay()
        torch.cuda.synchronize()
        first = [d.download() for d in ds]
        for d, m in zip(ds, c.members):
            d.rewrite(second_inputs(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        second = [d.download() for d in ds]
        del g
        own.release_captures()
        return first + second + ([run_refused(c.refused)] if c.refused else [])
    finally:
        own.close()


def run_refused(m):
    """m's call captured on a fresh context that reserved one block less than it has: the refusal's text (None when the
    call went through) under "rc", and every output as the refused call left it."""
    import kvsep
    import torch
    ctx = kvsep.Context(0)
    try:
        ctx.reserve(m.par["count"] - 1, m.nbytes + (1 << 20))
        d = Device(m)
        torch.cuda.synchronize()
        rc = None
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(ctx, d, torch.cuda.current_stream())
        except kvsep.KvsepError as e:
            rc = str(e)
        del g
        torch.cuda.synchronize()
        got = d.download()
        got["rc"] = rc
        return got
    finally:
        ctx.close()


def expect_refused(m):
    """A captured call over its reservation fails with KVSEP_EINVAL before anything is enqueued: nothing is written."""
    return {name: np.full(n, sentinel(dtype), dtype) for name, (dtype, n) in m.out.items()}


def second_inputs(m):
    """A case of the same shapes and parameters over other bytes: what a replay finds after its inputs were rewritten in
    place.  The payload is reversed, so every stored checksum of it is stale (the lists turn all-bad); a concat's segment
    CRCs, which are its whole input, are recomputed."""
    v = copy.copy(m)
    v.inp, v.host = dict(m.inp), dict(m.host)
    if m.form in ("sst_index", "sst_index_keys"):  # the walk alone trusts its block: the second handle leaves the image
        v.inp["handle"] = np.array([1 << 63, 1 << 63], np.uint64)
    elif "src" in m.inp:
        v.inp["src"] = m.inp["src"][::-1].copy()
    if m.form == "log_accept_gaps":  # the walk's arrays go with the image they were walked from
        r = _log_read(v, m.par["cap"])
        v.inp.update(w_off=r["off"], w_len=r["len"], w_type=r["type"], w_ok=r["ok"], w_nrec=r["nrec"])
    if m.form == "concat":
        v.host["src"] = m.host["src"][::-1].copy()
        v.inp["seg_crc"] = oracle().batch(v.host["src"], m.host["seg_off"], m.inp["seg_len"])
    return v


def check_case(ctx, c, stream=None):
    """run_case and compare against expect; raises Mismatch."""
    got = run_case(ctx, c, stream)
    if not c.members:
        compare(c, got, expect(c))
        return
    wants = expect(c)
    if c.family == "captured":
        wants = wants + [expect(second_inputs(m)) for m in c.members]
        members = c.members + [second_inputs(m) for m in c.members]
    else:
        members = c.members
    if c.refused:
        rc = got[-1].pop("rc")
        if rc is None or "(-1)" not in rc:
            raise Mismatch(f"{c.line()}: refused member {c.refused.line()}: rc = {rc} want KVSEP_EINVAL (-1)", "rc", 0)
        members, wants = members + [c.refused], wants + [expect_refused(c.refused)]
    for m, g, w in zip(members, got, wants):
        try:
            compare(m, g, w)
        except Mismatch as e:
            raise Mismatch(f"{c.line()}: member {e}", e.array, e.index) from None


def soak(seed, families=FAMILIES, seconds=None, max_cases=None, first=0, log=print):
    """Cases first, first + 1, ... of each family in turn until `seconds` elapse or max_cases ran per family; raises
    Mismatch on the first wrong result -> {family: (cases, elements)}."""
    import kvsep
    ctx = kvsep.Context(0)
    t_end = time.time() + seconds if seconds else float("inf")
    done = {f: [0, 0] for f in families}
    try:
        k = first
        while time.time() < t_end and (max_cases is None or k < first + max_cases):
            for f in families:
                c = make_case(f, seed, k)
                check_case(ctx, c)
                done[f][0] += 1
                done[f][1] += c.elements
                log(f"{c.line()} -> ok")
            k += 1
    finally:
        ctx.close()
    return {f: tuple(v) for f, v in done.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--seed", type=int, default=int(time.time()) & 0xFFFFFFFF)
    ap.add_argument("--family", choices=FAMILIES)
    ap.add_argument("--case", type=int, help="run this one case alone (with --family)")
    args = ap.parse_args()
    print(f"seed {args.seed}", flush=True)
    fams = (args.family,) if args.family else FAMILIES
    one = args.case is not None
    try:
        done = soak(args.seed, fams, seconds=None if one else args.seconds, max_cases=1 if one else None,
                    first=args.case if one else 0, log=lambda m: print(m, flush=True))
    except Mismatch as e:
        print(f"MISMATCH {e}", flush=True)
        sys.exit(1)
    print("soak ok: " + ", ".join(f"{f} {n} cases / {e} elements" for f, (n, e) in done.items()) +
          f", seed {args.seed}", flush=True)


if __name__ == "__main__":
    main()
