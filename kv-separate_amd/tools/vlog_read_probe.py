#!/usr/bin/env python3
"""What the device value-log reader costs (kvsep_vlog_walk_device, kvsep_vlog_read_device) against the path it
replaces, on three shapes:

  1mib    4,096 records of 1,048,609 bytes (config 3b's layout); only the headers are written, the payload is whatever
          the allocation holds, so every checksum fails -- the time does not depend on that
  100b    1,048,576 records of 100 bytes
  empty   1,048,576 empty records

Timed with events on one stream, after warm-up calls, median of --reps:

  walk      the walk kernel alone (kvsep_vlog_walk_device)
  read      the read form (walk, verify over cap elements, totals)
  verify    the verify call the read form contains (kvsep_crc32c_verify_device over the walked arrays)
  host      the path this replaces: D2H of the image into pinned memory, kvsep_vlog_walk on the host (the counting pass
            and the filling pass), H2D of the three arrays -- wall clock around a synchronise at each end

The window size is a compile-time constant of csrc/vlog_run.h; to compare window sizes build the library once per size
(make LIB=... BUILD=... CXXFLAGS='... -DKVSEP_VLOG_WINDOW=4096') and run this script once per library with --lib.

  python tools/vlog_read_probe.py [--lib PATH] [--reps 5] [--shapes 1mib,100b,empty]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kvsep  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"1mib": (4096, 1048609), "100b": (1 << 20, 100), "empty": (1 << 20, 0)}


def build(count, length):
    """The image on the device: headers at i * (8 + length), stored word i, the payload left as allocated."""
    rec = 8 + length
    n = count * rec
    d = torch.empty(n, dtype=torch.uint8, device=DEV)
    if length and n <= (1 << 30):
        kvsep.fill_splitmix64(d, n, 7)
    hdr = np.zeros((count, 2), np.uint32)
    hdr[:, 0] = np.arange(count, dtype=np.uint32) * np.uint32(2654435761)
    hdr[:, 1] = length
    pos = torch.arange(count, dtype=torch.int64, device=DEV) * rec
    idx = (pos[:, None] + torch.arange(8, dtype=torch.int64, device=DEV)[None, :]).reshape(-1)
    d[idx] = torch.from_numpy(hdr.view(np.uint8).reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    return d, n


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="a libkvsep_crc32c.so built with another KVSEP_VLOG_WINDOW")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1mib,100b,empty")
    ap.add_argument("--window", default="shipped", help="label only: the window the library was built with")
    args = ap.parse_args()
    if args.lib:
        kvsep.LIB_PATH = os.path.abspath(args.lib)
    ctx = kvsep.Context(0)
    print("# %s, window %s, %d reps, ms: median (min .. max)" % (torch.cuda.get_device_name(0), args.window, args.reps))
    for name in args.shapes.split(","):
        count, length = SHAPES[name]
        d, n = build(count, length)
        cap = count
        off = torch.zeros(cap, dtype=torch.int64, device=DEV)
        ln = torch.zeros(cap, dtype=torch.int64, device=DEV)
        st = torch.zeros(cap, dtype=torch.int32, device=DEV)
        crc = torch.zeros(cap, dtype=torch.int32, device=DEV)
        w = torch.zeros(8, dtype=torch.int64, device=DEV)
        ctx.reserve(cap, n)
        hint = max(length, 1)

        def walk():
            ctx.vlog_walk_device(d.data_ptr(), n, w[0:1], off=off, length=ln, stored=st, consumed=w[1:2], cap=cap)

        def read():
            ctx.vlog_read_device(d.data_ptr(), n, off, ln, st, crc, w[0:1], consumed=w[1:2], first_bad=w[2:3],
                                 nbad=w[3:4], ngood=w[4:5], good_bytes=w[5:6], drop_bytes=w[6:7], cap=cap,
                                 max_len_hint=hint)

        def verify():
            ctx.verify_device(d.data_ptr(), off, ln, st, crc, w[2:3], w[3:4], total_bytes=n, max_len=hint)

        pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)

        def host():
            pinned.copy_(d, non_blocking=True)
            torch.cuda.synchronize()
            h_off, h_len, h_st, _ = kvsep.vlog_walk(pinned.numpy())
            off.copy_(torch.from_numpy(h_off.view(np.int64)), non_blocking=True)
            ln.copy_(torch.from_numpy(h_len.view(np.int64)), non_blocking=True)
            st.copy_(torch.from_numpy(h_st.view(np.int32)), non_blocking=True)

        walk()
        torch.cuda.synchronize()
        assert int(w[0].item()) == count and int(w[1].item()) == n, "the walk did not find the records it was given"
        print("%-6s %9d records of %8d B, image %7.1f MiB" % (name, count, length, n / 2**20))
        for what, fn, t in (("walk", walk, timed), ("read", read, timed), ("verify", verify, timed),
                            ("host", host, wall)):
            med, lo, hi = t(fn, args.reps)
            print("  %-7s %10.3f  (%.3f .. %.3f)" % (what, med, lo, hi))
        del d, pinned
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
