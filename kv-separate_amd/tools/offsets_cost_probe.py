#!/usr/bin/env python3
"""What laying out on the device costs: the SST salvage form against the two existing calls it is made of.

Per shape four forms, each ONE hipGraph of K back-to-back calls timed with an event pair on the replay stream, the forms
interleaved over several rounds in one process, medians and runs per call reported (tools/frame_cost_probe.py does it
this way):
  verify   (a) kvsep_sst_verify_list_device alone, writing ok[]
  pack     (b) kvsep_crc32c_pack_device alone with offsets the host made: every block with its trailer, back to back
  offsets  (c) kvsep_crc32c_offsets_device alone (keep = ok[], tail = 5): the three small kernels
  salvage  (d) kvsep_sst_salvage_device whole
Expected: (d) ~ (a) + (b) + (c), and (c) ~ three launches.  `spread` is the largest distance of a run from its form's
median in the row: what a difference has to exceed to mean anything.
Shapes: a table of 65,536 x 4 KiB blocks and one of 4,096 x 64 KiB, each block followed by its 5-byte trailer (written by
kvsep_sst_frame_device), one block in 97 damaged.  The salvaged image is checked once against the table.

--ab PARENT_LIB measures the forms this change does not touch, kvsep_crc32c_verify_device and kvsep_crc32c_pack_device,
with the built library and with PARENT_LIB (a build of the parent commit) in alternating fresh processes.
usage: offsets_cost_probe.py [--steps 20] [--rounds 7] [--ab PARENT_LIB [--ab-rounds 3]]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--ab", default=None, help="the parent commit's library: measure the unchanged forms against it")
ap.add_argument("--ab-rounds", type=int, default=3)
ap.add_argument("--child", default=None, help="(internal) measure the unchanged forms with this library, one JSON line")
args = ap.parse_args()

KIB = 1 << 10
SHAPES = [("64Ki x 4 KiB", 65536, 4 * KIB), ("4Ki x 64 KiB", 4096, 64 * KIB)]

if args.ab:  # before this process touches the GPU: one child at a time, each a fresh process
    for r in range(args.ab_rounds):
        for name, path in (("built", None), ("parent", args.ab)) if r % 2 == 0 else (("parent", args.ab), ("built", None)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path or "built", "--steps", str(args.steps),
                   "--rounds", str(args.rounds)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode:
                sys.exit("child failed: " + out.stderr[-2000:])
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    print(json.dumps(dict(json.loads(line), library=name, process=r)), flush=True)

import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kvsep  # noqa: E402
from kvsep import workloads as W  # noqa: E402

if args.child and args.child != "built":  # an older library: bind what it has
    kvsep.LIB_PATH = args.child
    have = ctypes.CDLL(args.child)
    for n in [n for n in kvsep._SIGS if not hasattr(have, n)]:
        del kvsep._SIGS[n]

dev = torch.device("cuda:0")
u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)  # noqa: E731


def timed(graphs, forms):
    times = {f: [] for f in forms}
    for r in range(args.rounds):
        for form in (forms if r % 2 == 0 else forms[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[form].replay()
            e1.record()
            torch.cuda.synchronize()
            times[form].append(e0.elapsed_time(e1) * 1e3 / args.steps)  # us per call
    return times


def capture(call, forms):
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
    return graphs


rows = []
for shape, count, blk in SHAPES:
    tb = count * blk
    stride = blk + 5
    src_off = np.arange(count, dtype=np.uint64) * np.uint64(blk)
    ln = np.full(count, blk, np.uint64)
    tab_off = np.arange(count, dtype=np.uint64) * np.uint64(stride)
    data = torch.empty(tb + 64, dtype=torch.uint8, device=dev)
    kvsep.fill_splitmix64(data.data_ptr(), tb, W.SEED, 0)
    table = torch.zeros(count * stride + 64, dtype=torch.uint8, device=dev)
    dst = torch.zeros(count * stride + 64, dtype=torch.uint8, device=dev)
    ctx = kvsep.Context(0)
    ctx.reserve(count, tb + count)
    ctx.reserve_captures(6)
    d_tab, d_len = u64(tab_off), u64(ln)
    word = torch.zeros(count, dtype=torch.int32, device=dev)
    out = torch.zeros(count, dtype=torch.int32, device=dev)
    res = torch.zeros(4, dtype=torch.int64, device=dev)  # first_bad, nbad, end, nkept
    if args.child:  # the unchanged forms: verify_device over the blocks, pack_device of the blocks with trailer room
        d_src, d_first = u64(src_off), u64(np.arange(count + 1, dtype=np.uint64))
        ctx.batch_device(data.data_ptr(), d_src, d_len, out, total_bytes=tb, max_len=blk)
        torch.cuda.synchronize()
        crc = out.cpu().numpy().view(np.uint32).astype(np.uint64)
        masked = (((crc >> np.uint64(15)) | (crc << np.uint64(17))) + np.uint64(kvsep.MASK_DELTA)) & np.uint64(0xFFFFFFFF)
        stored = torch.from_numpy(masked.astype(np.uint32).view(np.int32)).to(dev)  # every block verifies

        def call(form, st):
            if form == "verify_device":
                ctx.verify_device(data.data_ptr(), d_src, d_len, stored, out, res[0:1], res[1:2], total_bytes=tb,
                                  max_len=blk, stream=st)
            else:
                ctx.pack_device(data.data_ptr(), d_src, d_len, d_first, dst.data_ptr(), count * stride, d_tab, stream=st)

        forms = ["verify_device", "pack_device"]
    else:
        types = torch.ones(count, dtype=torch.uint8, device=dev)
        ctx.sst_frame_device(data.data_ptr(), u64(src_off), d_len, types, word, table.data_ptr(), count * stride, d_tab,
                             total_bytes=tb, max_len=blk)
        torch.cuda.synchronize()
        bad = np.arange(48, count, 97)
        table[torch.from_numpy((tab_off[bad] + np.uint64(blk // 3)).astype(np.int64)).to(dev)] ^= 0x20
        kept = np.ones(count, bool)
        kept[bad] = False
        ok = torch.zeros(count, dtype=torch.uint8, device=dev)
        ok_fixed = torch.from_numpy(kept.astype(np.uint8)).to(dev)
        d_len5 = u64(np.where(kept, stride, 0))
        host_off = np.where(kept, np.cumsum(np.where(kept, stride, 0)) - stride, 2**64 - 1).astype(np.uint64)
        d_host_off, d_first = u64(host_off), u64(np.arange(count + 1, dtype=np.uint64))
        dst_p = torch.zeros(count * stride + 64, dtype=torch.uint8, device=dev)
        dst_off = torch.zeros(count, dtype=torch.int64, device=dev)
        dst_off_o = torch.zeros(count, dtype=torch.int64, device=dev)

        def call(form, st):
            if form == "verify":
                ctx.sst_verify_list_device(table.data_ptr(), d_tab, d_len, out, res[0:1], res[1:2], ok=ok,
                                           total_bytes=tb, max_len=blk, stream=st)
            elif form == "pack":
                ctx.pack_device(table.data_ptr(), d_tab, d_len5, d_first, dst_p.data_ptr(), count * stride, d_host_off,
                                stream=st)
            elif form == "offsets":
                ctx.offsets_device(d_len, dst_off_o, res[2:3], keep=ok_fixed, tail=5, nkept=res[3:4], stream=st)
            else:
                ctx.sst_salvage_device(table.data_ptr(), d_tab, d_len, out, ok, dst.data_ptr(), count * stride, dst_off,
                                       res[2:3], first_bad=res[0:1], nbad=res[1:2], nkept=res[3:4], total_bytes=tb,
                                       max_len=blk, stream=st)

        forms = ["verify", "pack", "offsets", "salvage"]
    graphs = capture(call, forms)
    times = timed(graphs, forms)
    med = {f: statistics.median(t) for f, t in times.items()}
    row = {"shape": shape, "blocks": count, "bytes": tb, "kernel": ctx.kernel_name(count, blk + 1, tb + count)}
    for f in forms:
        row[f + "_us"] = round(med[f], 2)
        row[f + "_runs_us"] = [round(t, 2) for t in times[f]]
    row["spread_us"] = round(max(abs(t - med[f]) for f in forms for t in times[f]), 2)
    if not args.child:
        nk = int(kept.sum())
        exact = res.tolist() == [int(bad[0]), bad.size, nk * stride, nk]
        exact = exact and torch.equal(dst[:nk * stride], dst_p[:nk * stride]) and torch.equal(dst_off, d_host_off)
        k = int(np.flatnonzero(kept)[-1])
        exact = exact and torch.equal(dst[(nk - 1) * stride:nk * stride], table[k * stride:(k + 1) * stride])
        row["exact"] = bool(exact)
        row["salvage_minus_parts_us"] = round(med["salvage"] - med["verify"] - med["pack"] - med["offsets"], 2)
        row["salvage_minus_verify_pack_us"] = round(med["salvage"] - med["verify"] - med["pack"], 2)
    print(json.dumps(row), flush=True)
    rows.append(row)
    del graphs
    torch.cuda.synchronize()
    ctx.release_captures()
    ctx.close()
    del data, table, dst
    torch.cuda.empty_cache()

if not args.child:
    print("%-13s %10s %9s %11s %11s %13s %13s %7s %6s" % ("shape", "(a) verify", "(b) pack", "(c) offsets", "(d) salvage",
                                                        "(d)-(a)-(b)", "(d)-(a)-(b)-(c)", "spread", "exact"))
    for r in rows:
        print("%-13s %10.2f %9.2f %11.2f %11.2f %13.2f %13.2f %7.2f %6s" % (
            r["shape"], r["verify_us"], r["pack_us"], r["offsets_us"], r["salvage_us"], r["salvage_minus_verify_pack_us"],
            r["salvage_minus_parts_us"], r["spread_us"], r["exact"]))
