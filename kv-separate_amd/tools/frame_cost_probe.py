#!/usr/bin/env python3
"""What the device write side costs: the gather-copy alone, against a plain device-to-device copy, and inside the frame
forms.

Per shape four forms, each ONE hipGraph of K back-to-back calls timed with an event pair on the replay stream, the forms
interleaved over several rounds in one process, medians and runs per call reported (tools/gather_cost_probe.py does it
this way):
  pack    (a) kvsep_crc32c_pack_device alone, the payload landing where the frame form puts it
  memcpy  (b) one device-to-device copy of the same byte count (torch's contiguous copy_: hipMemcpyAsync): the ceiling
  frame   (c) kvsep_vlog_frame_device / kvsep_sst_frame_device whole
  crc     (d) the CRC pass alone on the same descriptors: gather_device / sst_trailers_device
Expected: (c) - (d) ~ (a).  (a) / (b) says how far the kernel is from a copy; (d) / (c) is the share of the frame form a
copy fused into the CRC kernels could at most leave standing, i.e. 1 - (d) / (c) is the most fusion could save.
Shapes (source segments back to back from a 16-B aligned base, so `shift` is the payload's destination offset mod 16):
  4k x1 vlog   65,536 x 4 KiB, one segment each, records back to back (8-byte headers: shifts 8, 0, 8, ...)
  4k x1 sst    the same blocks as SST blocks back to back (5-byte trailers: every shift)
  4k x8 vlog   65,536 x 4 KiB as eight 512-B segments
  1m vlog      4,096 x 1 MiB, every payload at shift 8
  1m sst       4,096 x 1 MiB, every block at shift 0
  1g vlog      1 x 1 GiB at shift 8
Every form's output is checked once: the framed image's payload bytes against the source at three blocks, the header /
trailer words against the CRC pass.
usage: frame_cost_probe.py [--steps 20] [--rounds 7] [--shapes 4k,1m,1g]"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kvsep  # noqa: E402
from kvsep import workloads as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--shapes", default="4k,1m,1g")
args = ap.parse_args()
dev = torch.device("cuda:0")
u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)  # noqa: E731

KIB, MIB = 1 << 10, 1 << 20
# (name, group, blocks, block bytes, segments per block, frame, record stride - block bytes, payload offset in record)
SHAPES = [("4k x1 vlog", "4k", 65536, 4 * KIB, 1, "vlog", 8, 8), ("4k x1 sst", "4k", 65536, 4 * KIB, 1, "sst", 5, 0),
          ("4k x8 vlog", "4k", 65536, 4 * KIB, 8, "vlog", 8, 8), ("1m vlog", "1m", 4096, MIB, 1, "vlog", 16, 8),
          ("1m sst", "1m", 4096, MIB, 1, "sst", 16, 0), ("1g vlog", "1g", 1, 1 << 30, 1, "vlog", 16, 8)]
rows = []
for shape, group, count, blk, per_block, frame, pad, lead in SHAPES:
    if group not in args.shapes.split(","):
        continue
    nseg, seg, tb = count * per_block, blk // per_block, count * blk
    seg_off = np.arange(nseg, dtype=np.uint64) * np.uint64(seg)
    seg_len = np.full(nseg, seg, np.uint64)
    first = np.arange(count + 1, dtype=np.uint64) * np.uint64(per_block)
    rec_off = np.arange(count, dtype=np.uint64) * np.uint64(blk + pad)
    dst_bytes = count * (blk + pad)
    data = torch.empty(tb + 64, dtype=torch.uint8, device=dev)
    kvsep.fill_splitmix64(data.data_ptr(), tb, W.SEED, 0)
    dst = torch.zeros(dst_bytes + 64, dtype=torch.uint8, device=dev)
    dst_p = torch.zeros(dst_bytes + 64, dtype=torch.uint8, device=dev)
    d_off, d_len, d_first, d_rec, d_pay = u64(seg_off), u64(seg_len), u64(first), u64(rec_off), u64(rec_off + np.uint64(lead))
    types = torch.ones(count, dtype=torch.uint8, device=dev)
    ctx = kvsep.Context(0)
    ctx.reserve(nseg, tb)
    ctx.reserve_captures(4)
    seg_crc = torch.zeros(nseg, dtype=torch.int32, device=dev)
    seg_crc_d = torch.zeros(nseg, dtype=torch.int32, device=dev)
    word = torch.zeros(count, dtype=torch.int32, device=dev)
    word_d = torch.zeros(count, dtype=torch.int32, device=dev)

    def call(form, st):
        if form == "pack":
            ctx.pack_device(data.data_ptr(), d_off, d_len, d_first, dst_p.data_ptr(), dst_bytes, d_pay, stream=st)
        elif form == "memcpy":
            dst_p[:tb].copy_(data[:tb], non_blocking=True)
        elif form == "frame" and frame == "vlog":
            ctx.vlog_frame_device(data.data_ptr(), d_off, d_len, d_first, seg_crc, word, dst.data_ptr(), dst_bytes, d_rec,
                                  total_bytes=tb, max_len=seg, stream=st)
        elif form == "frame":
            ctx.sst_frame_device(data.data_ptr(), d_off, d_len, types, word, dst.data_ptr(), dst_bytes, d_rec,
                                 total_bytes=tb, max_len=seg, stream=st)
        elif frame == "vlog":
            ctx.gather_device(data.data_ptr(), d_off, d_len, d_first, seg_crc_d, word_d, total_bytes=tb, max_len=seg,
                              stream=st)
        else:
            ctx.sst_trailers_device(data.data_ptr(), d_off, d_len, types, word_d, total_bytes=tb, max_len=seg, stream=st)

    forms = ["pack", "memcpy", "frame", "crc"]
    graphs = {}
    for form in forms:
        call(form, torch.cuda.current_stream())
        torch.cuda.synchronize()
        if form == "pack":  # checked before the copy overwrites dst_p
            exact = all(torch.equal(dst_p[int(rec_off[i]) + lead:int(rec_off[i]) + lead + blk], data[i * blk:(i + 1) * blk])
                        for i in {0, count // 2, count - 1})
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.steps):
                call(form, torch.cuda.current_stream())
        g.replay()
        torch.cuda.synchronize()
        graphs[form] = g
    for i in {0, count // 2, count - 1}:
        r0 = int(rec_off[i])
        exact = exact and torch.equal(dst[r0 + lead:r0 + lead + blk], data[i * blk:(i + 1) * blk])
        w = int(word_d[i].item()) & 0xFFFFFFFF
        if frame == "vlog":
            head = dst[r0:r0 + 8].cpu().numpy().view("<u4")
            exact = exact and int(head[0]) == kvsep.mask(w) and int(head[1]) == blk
        else:
            tail = dst[r0 + blk:r0 + blk + 5].cpu().numpy()
            exact = exact and int(tail[0]) == 1 and int(tail[1:].copy().view("<u4")[0]) == w
    exact = bool(exact and torch.equal(word, word_d))
    times = {f: [] for f in forms}
    for r in range(args.rounds):
        for form in (forms if r % 2 == 0 else forms[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[form].replay()
            e1.record()
            torch.cuda.synchronize()
            times[form].append(e0.elapsed_time(e1) * 1e3 / args.steps)  # us per call
    med = {f: statistics.median(t) for f, t in times.items()}
    row = {"shape": shape, "segments": nseg, "blocks": count, "bytes": tb, "kernel": ctx.kernel_name(nseg, seg, tb),
           "exact": exact}
    for f in forms:
        row[f + "_us"] = round(med[f], 2)
        row[f + "_runs_us"] = [round(t, 2) for t in times[f]]
    row["pack_over_memcpy"] = round(med["pack"] / med["memcpy"], 3)
    row["frame_minus_crc_us"] = round(med["frame"] - med["crc"], 2)
    row["crc_over_frame"] = round(med["crc"] / med["frame"], 3)
    row["pack_tb_per_s"] = round(2 * tb / med["pack"] / 1e6, 3)  # bytes read + bytes written
    print(json.dumps(row), flush=True)
    rows.append(row)
    del graphs, g
    torch.cuda.synchronize()
    ctx.release_captures()
    ctx.close()
    del data, dst, dst_p
    torch.cuda.empty_cache()

print("%-11s %9s %9s %9s %9s %9s %7s %7s %6s" % ("shape", "(a) pack", "(b) copy", "(c) frame", "(d) crc", "(c)-(d)",
                                                 "(a)/(b)", "(d)/(c)", "exact"))
for r in rows:
    print("%-11s %9.2f %9.2f %9.2f %9.2f %9.2f %7.3f %7.3f %6s" % (
        r["shape"], r["pack_us"], r["memcpy_us"], r["frame_us"], r["crc_us"], r["frame_minus_crc_us"],
        r["pack_over_memcpy"], r["crc_over_frame"], r["exact"]))
