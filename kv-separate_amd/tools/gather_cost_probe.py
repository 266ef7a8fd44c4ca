#!/usr/bin/env python3
"""What the gather form costs over the batch form on the very same segment list.

kvsep_crc32c_gather_device is kvsep_crc32c_batch_device over the segments followed by crc32c_concat_kernel, so "batch"
(existing code) is the yardstick and gather - batch is the concat pass; "concat" times kvsep_crc32c_concat_device alone
on the segment CRCs the batch form left.  Each form is ONE hipGraph of K back-to-back calls timed with an event pair on
the replay stream, the forms interleaved over several rounds in one process, medians and runs per call reported
(tools/verify_cost_probe.py --list-cost does it this way).  Shapes:
  4k x1    65,536 x 4 KiB segments, one per block: the concat pass should cost about a launch
  4k x8    the same segments, eight per block
  128 x64  1,048,576 x 128-B segments, 64 per block: the most segments per payload byte; runs over the short / long
           threshold (concat_run.h), so every block takes the wavefront path
Every form's output is checked once: the gather form's block CRCs against batch_device over the blocks' contiguous bytes
(the segments of a block lie back to back here), its seg_crc against the batch form's.
usage: gather_cost_probe.py [--steps 20] [--rounds 7]"""
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
args = ap.parse_args()
dev = torch.device("cuda:0")
u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)  # noqa: E731

for shape, nseg, seg, per_block in (("4k x1", 65536, 4096, 1), ("4k x8", 65536, 4096, 8), ("128 x64", 1 << 20, 128, 64)):
    count, tb = nseg // per_block, nseg * seg
    seg_off = np.arange(nseg, dtype=np.uint64) * np.uint64(seg)
    seg_len = np.full(nseg, seg, np.uint64)
    first = np.arange(count + 1, dtype=np.uint64) * np.uint64(per_block)
    data = torch.empty(tb + 64, dtype=torch.uint8, device=dev)
    kvsep.fill_splitmix64(data.data_ptr(), tb, W.SEED, 0)
    d_off, d_len, d_first = u64(seg_off), u64(seg_len), u64(first)
    ctx = kvsep.Context(0)
    ctx.reserve(nseg, tb)
    ctx.reserve_captures(4)
    seg_crc = torch.zeros(nseg, dtype=torch.int32, device=dev)
    seg_crc_b = torch.zeros(nseg, dtype=torch.int32, device=dev)
    out = torch.zeros(count, dtype=torch.int32, device=dev)
    out_c = torch.zeros(count, dtype=torch.int32, device=dev)
    whole = torch.zeros(count, dtype=torch.int32, device=dev)
    ctx.batch_device(data.data_ptr(), u64(first[:-1] * np.uint64(seg)), u64(np.full(count, seg * per_block)), whole,
                     total_bytes=tb, max_len=seg * per_block)

    def call(form, st):
        if form == "batch":
            ctx.batch_device(data.data_ptr(), d_off, d_len, seg_crc_b, total_bytes=tb, max_len=seg, stream=st)
        elif form == "gather":
            ctx.gather_device(data.data_ptr(), d_off, d_len, d_first, seg_crc, out, total_bytes=tb, max_len=seg,
                              stream=st)
        else:
            ctx.concat_device(seg_crc_b, d_len, d_first, out_c, stream=st)

    forms = ["batch", "gather", "concat"]
    graphs = {}
    for form in forms:
        call(form, torch.cuda.current_stream())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.steps):
                call(form, torch.cuda.current_stream())
        g.replay()
        torch.cuda.synchronize()
        graphs[form] = g
    exact = bool(torch.equal(out, whole) and torch.equal(out_c, whole) and torch.equal(seg_crc, seg_crc_b))
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
    row["gather_over_batch"] = round(med["gather"] / med["batch"], 4)
    row["gather_minus_batch_us"] = round(med["gather"] - med["batch"], 2)
    row["concat_over_batch"] = round(med["concat"] / med["batch"], 4)
    print(json.dumps(row), flush=True)
    del graphs, g
    torch.cuda.synchronize()
    ctx.release_captures()
    ctx.close()
    del data
    torch.cuda.empty_cache()
