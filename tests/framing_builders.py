"""Reference-format image builders for the framing tests -- TEST INFRASTRUCTURE, checksums from the
oracle.  Each follows the reference writer it names, so the engine's walkers/verifiers are checked
against independently framed bytes."""
import struct

import numpy as np


def vlog_image(payloads, oracle):
    """db/value_log_writer.cc:46-76: [Mask(Value(p)) LE32][len LE32][p] back to back."""
    out = bytearray()
    for p in payloads:
        c = oracle.lib.oracle_crc32c_mask(oracle.extend(0, p))
        out += struct.pack("<II", c, len(p)) + p
    return bytes(out)


BLOCK, HEADER = 32768, 7  # db/log_format.h:30,33
FULL, FIRST, MIDDLE, LAST = 1, 2, 3, 4


def log_image(records, oracle):
    """log::Writer::AddRecord (db/log_writer.cc:35-82) + EmitPhysicalRecord (:84-115).
    Returns (image, physical) with physical = [(header_offset, type, payload_len)]."""
    out = bytearray()
    phys = []
    block_off = 0
    for rec in records:
        left, pos, begin = len(rec), 0, True
        while True:
            leftover = BLOCK - block_off
            if leftover < HEADER:
                out += b"\x00" * leftover
                block_off = 0
            avail = BLOCK - block_off - HEADER
            frag = min(left, avail)
            end = left == frag
            t = FULL if (begin and end) else FIRST if begin else LAST if end else MIDDLE
            data = rec[pos:pos + frag]
            crc = oracle.lib.oracle_crc32c_mask(oracle.extend(oracle.extend(0, bytes([t])), data))
            phys.append((len(out), t, frag))
            out += struct.pack("<IHB", crc, frag, t) + data
            block_off += HEADER + frag
            pos += frag
            left -= frag
            begin = False
            if left == 0:
                break
    return bytes(out), phys


_FNV = {}


def fnv64(b: bytes) -> str:
    """The record identity of tests/golden/*.json (FNV-1a 64, independent of the CRC under test); cached per content,
    since most records of a damaged file are those of the intact one."""
    h = _FNV.get(b)
    if h is None:
        x = 0xCBF29CE484222325
        for c in b:
            x = ((x ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        h = _FNV[b] = "%016x" % x
    return h


def assemble(img, off, ln, ty, accept, gap=None):
    """log::Reader::ReadRecord (db/log_reader.cc:58-173) over the physical records of kvsep_log_walk: FULL returns,
    FIRST/MIDDLE/LAST assemble; a dropped record (accept 0), a reader event without a record before this one
    (gap 1: bad record length or zero header, kvsep_log_accept_gaps) and an unknown type each abandon the record in
    progress, as kBadRecord / "unknown record type" do.  -> [[len, fnv64], ...] of the logical records."""
    out, scratch, infrag = [], b"", False
    if gap is None:
        gap = [0] * len(accept)
    for o, n, t, a, g in zip(off, ln, ty, accept, gap):
        frag = img[int(o) + 1:int(o) + int(n)]  # off points at the type byte, len = 1 + payload
        if g or not a:
            infrag, scratch = False, b""
        if not a:
            continue
        if t == FULL:
            infrag, scratch = False, b""
            out.append(frag)
        elif t == FIRST:
            scratch, infrag = frag, True
        elif t == MIDDLE:
            if infrag:
                scratch += frag
        elif t == LAST:
            if infrag:
                out.append(scratch + frag)
                infrag, scratch = False, b""
        else:
            infrag, scratch = False, b""
    return [[len(r), fnv64(r)] for r in out]


def sst_image(blocks, types, oracle):
    """TableBuilder::WriteRawBlock (table/table_builder.cc:209-232): block, then [type][Mask(crc)]
    with crc = Extend(Value(block), &type, 1).  Returns (image, offsets, trailer words)."""
    out = bytearray()
    offs, words = [], []
    for b, t in zip(blocks, types):
        crc = oracle.extend(oracle.extend(0, b), bytes([t]))
        w = oracle.lib.oracle_crc32c_mask(crc)
        offs.append(len(out))
        words.append(w)
        out += b + bytes([t]) + struct.pack("<I", w)
    return bytes(out), np.array(offs, np.uint64), np.array(words, np.uint32)


def writer(lens, keep, dest_length):
    """log::Writer::AddRecord (db/log_writer.cc:35-82) over the kept lengths, from block offset dest_length % 32768:
    ([(header offset, type, fragment length, record, position in the record)], [(pad offset, pad bytes, record)],
    bytes appended)."""
    phys, pads, pos, block_off = [], [], 0, dest_length % BLOCK
    for r, n in enumerate(lens):
        if not keep[r]:
            continue
        left, at, begin = int(n), 0, True
        while True:
            leftover = BLOCK - block_off
            if leftover < HEADER:
                if leftover:
                    pads.append((pos, leftover, r))
                pos += leftover
                block_off = 0
            frag = min(left, BLOCK - block_off - HEADER)
            end = left == frag
            phys.append((pos, FULL if begin and end else FIRST if begin else LAST if end else MIDDLE, frag, r, at))
            pos += HEADER + frag
            block_off += HEADER + frag
            at += frag
            left -= frag
            begin = False
            if left == 0:
                break
    return phys, pads, pos


M64 = 0xFFFFFFFFFFFFFFFF
SKIP = M64  # KVSEP_OFFSET_SKIP


def sat(a, b):
    return min(a + b, M64)


def ref_offsets(seg_len, first, keep, before, head, tail, start, max_size, count):
    """dst_off, end, nkept by the serial loop of crc32c_offsets.inc's header comment."""
    pos, nk, out, kept_segs = start, 0, [], set()
    for i in range(count):
        kept = (keep is None or keep[i] != 0) and (before is None or i < before)
        if not kept:
            out.append(SKIP)
            continue
        s, e = (int(first[i]), int(first[i + 1])) if first is not None else (i, i + 1)
        size = 0
        for j in range(s, e):
            size = sat(size, int(seg_len[j]))
            kept_segs.add(j)
        if size > max_size:
            size = M64
        ext = sat(sat(head, size), tail)
        end = sat(pos, ext)
        out.append(end - ext if end != M64 else SKIP)
        pos = end
        nk += 1
    return np.array(out, np.uint64), pos, nk, kept_segs


def log_scan(img):
    """log::Reader::ReadPhysicalRecord's parse of an image (db/log_reader.cc:189-243), block by block, in order:
    ("rec", header offset, payload length, type, stored word) for a physical record, ("skip", offset, block end, zero)
    where the reader gives up the rest of a block buffer: a length past its end, or a zero header (zero = True).  Fewer
    than 7 bytes left in a block are a trailer and are not read."""
    n, out = len(img), []
    for begin in range(0, n, BLOCK):
        end, p = min(begin + BLOCK, n), begin
        while end - p >= HEADER:
            stored, ln, t = struct.unpack_from("<IHB", img, p)
            if HEADER + ln > end - p:
                out.append(("skip", p, end, False))
                break
            if t == 0 and ln == 0:
                out.append(("skip", p, end, True))
                break
            out.append(("rec", p, ln, t, stored))
            p += HEADER + ln
    return out


def log_accept(events, n, ok, count):
    """What log::Reader makes of the first `count` physical records of log_scan, given their checksum verdicts ->
    (accept, gap, bytes reported with "checksum mismatch", bytes reported with "bad record length").  A mismatch drops
    the rest of its block buffer (:250-258); a good record of type 5 reads as kEof and ends the reading, type 6 as a
    kBadRecord nobody reports (:270-271); a skip the reader reaches marks the next record it reads (gap) and, for a
    bad length in a block that was read in full, is reported (:224-235)."""
    accept, gap = [0] * count, [0] * count
    i, dropped, bad_length, dead, pending, stopped = 0, 0, 0, -1, False, False
    for e in events:
        blk = e[1] // BLOCK
        if e[0] == "skip":
            if not stopped and blk != dead:
                pending = True
                if not e[3] and e[2] - blk * BLOCK == BLOCK:
                    bad_length += e[2] - e[1]
            continue
        k, i = i, i + 1
        if k >= count or stopped or blk == dead:
            continue
        gap[k], pending = int(pending), False
        if not ok[k]:
            dropped += min((blk + 1) * BLOCK, n) - e[1]
            dead = blk
        elif e[3] == 5:
            stopped = True
        else:
            accept[k] = int(e[3] != 6)
    return accept, gap, dropped, bad_length


def log_chain_table(ty, accept, gap):
    """The rule table of include/kvsep_crc32c.h for kvsep_log_chains, restated: (first, whole, nchain) with padding."""
    count = len(ty)
    first, whole, state_in = [], [], False
    continued = False
    for i in range(count):
        t, a, g = int(ty[i]), int(accept[i]), int(gap[i])
        if not a:
            cont, after = False, False
        elif t == FIRST:
            cont, after = False, True
        elif t == MIDDLE and not g:
            cont, after = state_in, state_in
        elif t == MIDDLE:
            cont, after = False, False
        elif t == LAST:
            cont, after = (not g) and state_in, False
        else:
            cont, after = False, False
        if not cont:
            first.append(i)
            whole.append(0)
        continued = cont
        # the chain is whole iff its last record is an accepted FULL or a LAST that continued: the latest record decides
        whole[-1] = 1 if a and (t == FULL or (t == LAST and continued)) else 0
        state_in = after
    nchain = len(first)
    return first + [count] * (count + 1 - nchain), whole + [0] * (count - nchain), nchain
