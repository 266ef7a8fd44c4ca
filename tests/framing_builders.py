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
