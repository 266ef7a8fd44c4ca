#!/usr/bin/env python3
"""What a device-resident SST table costs to check, from bytes to a per-block verdict list:

  table   kvsep_sst_table_verify_device: footer, index read check, index walk, read check and list pass, one stream;
  walk    kvsep_sst_index_device alone, from the index handle on the device;
  before  the route such a table had before: D2H of the footer and the caller's own decode of it, D2H of the index
          block and its parse on the host (kvsep_sst_index_walk, the fastest host parse there is), H2D of off[] /
          len[], then kvsep_sst_verify_list_device.

Event pairs around warm calls, the forms interleaved in one process, medians of 9 with the range; the verdicts of the
two routes are compared.  Shapes: the reference's tests/golden/ref_table.sst and a synthetic table of 65,536 x 4 KiB
blocks laid out below the way TableBuilder lays one out (index block at restart interval 1).

  python tools/sst_table_probe.py [--out FILE] [--blocks 65536] [--block-bytes 4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kvsep  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 9


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def trailer(block):
    """[type 0][Mask(Value(block || type)) LE32] (table/table_builder.cc:209-232)."""
    return b"\0" + kvsep.mask(kvsep.extend(kvsep.value(block), b"\0")).to_bytes(4, "little")


def build_table(nblocks, block_bytes, seed=7):
    """Data blocks of pseudo-random bytes with their trailers, an empty metaindex block, an index block with every
    entry a restart point (shared = 0), the footer."""
    payload = kvsep.splitmix64_bytes(nblocks * block_bytes, seed, 0).tobytes()
    parts, index, restarts, p = [], bytearray(), [], 0
    for i in range(nblocks):
        blk = payload[i * block_bytes:(i + 1) * block_bytes]
        parts += [blk, trailer(blk)]
        key, val = b"key%010d" % i + bytes(8), varint(p) + varint(block_bytes)
        restarts.append(len(index))
        index += varint(0) + varint(len(key)) + varint(len(val)) + key + val
        p += block_bytes + 5
    tail = lambda rs: b"".join(r.to_bytes(4, "little") for r in rs) + len(rs).to_bytes(4, "little")
    meta = tail([0])
    index = bytes(index) + tail(restarts or [0])
    foot = varint(p) + varint(len(meta)) + varint(p + len(meta) + 5) + varint(len(index))
    parts += [meta, trailer(meta), index, trailer(index), foot + bytes(40 - len(foot)),
              (0xdb4775248b80fb57).to_bytes(8, "little")]
    return b"".join(parts)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0  # us


def probe(name, img, max_len, out):
    n = len(img)
    (moff, mlen, ioff, ilen), st = kvsep.sst_footer(img)
    assert st == kvsep.SST_OK
    nblocks = kvsep.sst_index_walk(img[ioff:ioff + ilen])[2]
    cap = nblocks + 2
    ctx = kvsep.Context(0)
    ctx.reserve(max(cap, ilen // 4), n)
    d = torch.from_numpy(np.frombuffer(bytes(img), np.uint8).copy()).to(DEV)
    i64 = lambda k, v=0: torch.full((k,), v, dtype=torch.int64, device=DEV)
    off, ln, bad_idx, words, handles = i64(cap), i64(cap), i64(cap), i64(3), i64(4)
    crc = torch.zeros(cap, dtype=torch.int32, device=DEV)
    ok = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    off2, ln2, bad2, words2 = i64(cap), i64(cap), i64(cap), i64(2)
    crc2 = torch.zeros(cap, dtype=torch.int32, device=DEV)
    ok2 = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    handle = torch.tensor([ioff, ilen], dtype=torch.int64, device=DEV)
    h_foot = torch.empty(48, dtype=torch.uint8).pin_memory()
    h_index = torch.empty(ilen, dtype=torch.uint8).pin_memory()
    h_off = torch.empty(cap, dtype=torch.int64).pin_memory()
    h_len = torch.empty(cap, dtype=torch.int64).pin_memory()

    def table():
        ctx.sst_table_verify_device(d.data_ptr(), n, off, ln, crc, ok, words[0:1], handles, status,
                                    first_bad=words[1:2], nbad=words[2:3], bad_idx=bad_idx, cap=cap,
                                    max_len_hint=max_len)

    def walk():
        ctx.sst_index_device(d.data_ptr(), n, handle, off2, ln2, words2[0:1], status, cap=cap)

    def before():
        h_foot.copy_(d[n - 48:], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        # the caller's own footer parse (table/format.cc:37-60), as INTEGRATION.md had it before: the magic, four
        # varint64, both handles inside the n bytes
        foot = h_foot.numpy().tobytes()
        assert int.from_bytes(foot[40:], "little") == 0xdb4775248b80fb57
        hs, at = [], 0
        for _ in range(4):
            v = shift = 0
            while True:
                b = foot[at]
                at += 1
                v |= (b & 127) << shift
                shift += 7
                if b < 128:
                    break
            hs.append(v)
        mo, ml, io, il = hs
        assert mo + ml + 5 <= n and io + il + 5 <= n
        h_index.copy_(d[io:io + il], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        o, k, cnt, s = kvsep.sst_index_walk(h_index.numpy())
        h_off[:cnt] = torch.from_numpy(o.view(np.int64))
        h_len[:cnt] = torch.from_numpy(k.view(np.int64))
        h_off[cnt], h_len[cnt], h_off[cnt + 1], h_len[cnt + 1] = mo, ml, io, il
        off2.copy_(h_off, non_blocking=True)
        ln2.copy_(h_len, non_blocking=True)
        ctx.sst_verify_list_device(d.data_ptr(), off2, ln2, crc2, first_bad=words2[0:1], nbad=words2[1:2],
                                   bad_idx=bad2, ok=ok2, total_bytes=n, max_len=max_len)

    forms = {"table": table, "walk": walk, "before": before}
    for f in forms.values():  # warm
        f()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, f in forms.items():
            times[k].append(timed(f))
    torch.cuda.synchronize()
    same = (torch.equal(off, off2) and torch.equal(ln, ln2) and torch.equal(crc, crc2) and torch.equal(ok, ok2) and
            int(words[0]) == nblocks and int(status[0]) == kvsep.SST_OK and int(words[2]) == int(words2[1]))
    out.write(f"{name}: {n} bytes, {nblocks} data blocks, index block {ilen} bytes; outputs of both routes equal: "
              f"{same}\n")
    for k, v in times.items():
        out.write(f"  {k:7s} median {statistics.median(v):9.1f} us   range {min(v):9.1f} .. {max(v):9.1f}  (n={ROUNDS})\n")
    ctx.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--block-bytes", type=int, default=4096)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    golden = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests", "golden", "ref_table.sst")
    with open(golden, "rb") as f:
        ok = probe("reference table", f.read(), 4300, out)
    ok = probe(f"synthetic {a.blocks} x {a.block_bytes} B", build_table(a.blocks, a.block_bytes), a.block_bytes,
               out) and ok
    out.flush()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
