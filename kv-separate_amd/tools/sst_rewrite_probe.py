#!/usr/bin/env python3
"""What finishing a salvaged SST table on the device costs:

  build    kvsep_sst_index_build_device alone over `count` entries of 21-byte keys (count = 1,024 and 65,536), against
           a device-to-device copy of the index block's bytes (the floor of any way to produce it);
  rewrite  kvsep_sst_table_rewrite_device of a 65,536 x 4 KiB table with a few bad blocks, against
           kvsep_sst_table_verify_device followed by kvsep_sst_salvage_device on the same table (what was there before,
           which leaves no index block, metaindex block or footer), and against the salvage alone.

Event pairs around warm calls, the forms interleaved in one process, medians of 9 with the range; the rewrite's output
is checked with the table verify before it is timed.

  python tools/sst_rewrite_probe.py [--out FILE] [--blocks 65536] [--block-bytes 4096]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import kvsep  # noqa: E402
from sst_table_probe import build_table, timed  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 9


def report(out, times):
    for k, v in times.items():
        out.write(f"  {k:14s} median {statistics.median(v):9.1f} us   range {min(v):9.1f} .. {max(v):9.1f}  (n={ROUNDS})\n")


def interleave(forms):
    for f in forms.values():  # warm
        f()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, f in forms.items():
            times[k].append(timed(f))
    torch.cuda.synchronize()
    return times


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).to(DEV)


def probe_build(count, out):
    keys = b"".join(b"key%010d" % i + bytes(8) for i in range(count))
    ko = np.arange(count, dtype=np.uint64) * 21
    kl = np.full(count, 21, np.uint64)
    bo = np.arange(count, dtype=np.uint64) * 4101
    bl = np.full(count, 4096, np.uint64)
    want, want_len, st = kvsep.sst_index_build(keys, ko, kl, bo, bl)
    assert st == kvsep.SSTW_OK
    ctx = kvsep.Context(0)
    ctx.reserve(count, len(want) + 64)
    src = torch.from_numpy(np.frombuffer(keys, np.uint8).copy()).to(DEV)
    dko, dkl, dbo, dbl = i64(ko), i64(kl), i64(bo), i64(bl)
    dst = torch.zeros(len(want) + 64, dtype=torch.uint8, device=DEV)
    dst2 = torch.zeros_like(dst)
    at = i64([0])
    res = torch.zeros(1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def build():
        ctx.sst_index_build_device(src.data_ptr(), dko, dkl, dbo, dbl, dst.data_ptr(), dst.numel(), at, res, status)

    def copy():
        dst2[:len(want)].copy_(dst[:len(want)])

    times = interleave({"build": build, "d2d copy": copy})
    same = dst[:len(want)].cpu().numpy().tobytes() == want and int(status[0]) == 0
    out.write(f"index build, {count} entries of 21-byte keys: block {want_len} bytes; equal to the host form: {same}\n")
    report(out, times)
    ctx.close()
    return same


def probe_rewrite(nblocks, block_bytes, out):
    img = bytearray(build_table(nblocks, block_bytes))
    n = len(img)
    for i in (0, nblocks // 3, nblocks - 1):
        img[i * (block_bytes + 5) + 17] ^= 0x20
    cap = nblocks + 2
    (_, _, ioff, ilen), _ = kvsep.sst_footer(bytes(img))
    ctx = kvsep.Context(0)
    ctx.reserve(max(cap, ilen // 4), 2 * n)
    d = torch.from_numpy(np.frombuffer(bytes(img), np.uint8).copy()).to(DEV)
    z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=DEV)
    off, ln, ko, kl, dst_off = (z(cap) for _ in range(5))
    crc, ok = z(cap, torch.int32), z(cap, torch.uint8)
    words, st = z(12), z(2, torch.int32)
    dst = z(n, torch.uint8)
    dst2 = z(n, torch.uint8)

    def rewrite():
        ctx.sst_table_rewrite_device(d.data_ptr(), n, dst.data_ptr(), n, off, ln, ko, kl, crc, ok, dst_off, words[0:1],
                                     words[4:8], st[0:1], words[2:3], words[3:4], st[1:2], nkept=words[1:2], cap=cap,
                                     max_len_hint=block_bytes)

    def verify():
        ctx.sst_table_verify_device(d.data_ptr(), n, off, ln, crc, ok, words[0:1], words[4:8], st[0:1],
                                    first_bad=words[8:9], nbad=words[9:10], cap=cap, max_len_hint=block_bytes)

    def salvage():
        ctx.sst_salvage_device(d.data_ptr(), off, ln, crc, ok, dst2.data_ptr(), n, dst_off, words[10:11],
                               nkept=words[11:12], count=cap, total_bytes=n, max_len=block_bytes)

    def verify_salvage():
        verify()
        salvage()

    rewrite()
    torch.cuda.synchronize()
    tb, nk = int(words[3]), int(words[1])
    o2, l2, c2, k2, w2, s2 = z(cap), z(cap), z(cap, torch.int32), z(cap, torch.uint8), z(8), z(1, torch.int32)
    ctx.sst_table_verify_device(dst.data_ptr(), tb, o2, l2, c2, k2, w2[0:1], w2[4:8], s2, first_bad=w2[1:2],
                                nbad=w2[2:3], cap=cap)
    torch.cuda.synchronize()
    good = (st.tolist() == [0, 0] and nk == nblocks - 3 and int(s2[0]) == 0 and int(w2[0]) == nk and int(w2[2]) == 0)
    verify()  # the salvage's inputs
    times = interleave({"rewrite": rewrite, "verify+salvage": verify_salvage, "salvage": salvage})
    out.write(f"rewrite, {nblocks} x {block_bytes} B, 3 bad blocks: {n} -> {tb} bytes, index block {ilen} bytes; the "
              f"output verifies as a clean table of {nk} blocks: {good}\n")
    report(out, times)
    ctx.close()
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--block-bytes", type=int, default=4096)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    ok = probe_build(1024, out)
    ok = probe_build(65536, out) and ok
    ok = probe_rewrite(a.blocks, a.block_bytes, out) and ok
    out.flush()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
