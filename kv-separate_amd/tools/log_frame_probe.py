#!/usr/bin/env python3
"""What writing a log / MANIFEST image from device-resident records costs: kvsep_log_frame_device against the route
such a batch had without it.

Per shape the forms below, interleaved over the rounds in one process, each timed with an event pair on the stream (the
host steps of `host` lie between the events, so the pair spans them), medians and runs reported:
  frame   kvsep_log_frame_device: layout, fragment fill, checksums and the framed copy on the stream, no host step
  host    D2H of the records, kvsep_log_frame_host, H2D of the image
  layout  the call with frag_cap = 0 and dst_bytes = 0: the layout kernel and an idle fill, the one serial piece
  crc     kvsep_crc32c_batch_device over the fragment descriptors the call left (max_len 32,761)
  copy    kvsep_crc32c_pack_device over the same descriptors (the plain frame: the copy less the 7-byte headers)
Shapes:
  1k      65,536 records of 1 KiB
  100k    655 records of 100 KiB
  ref     the 12 records of tests/golden/ref_manifest.log, when tests/golden is there
The images of `frame` and `host` are compared once.  Then the layout alone at 65,536 and 1,048,576 records of 1 KiB
(lengths only: nothing is read or written but the arrays).
usage: log_frame_probe.py [--rounds 9] [--shapes 1k,100k,ref] [--unchanged] [--lib PATH]
  --unchanged   time pack_device and vlog_frame_device alone (one JSON line each): for A/B runs against another build
  --lib PATH    load that libkvsep_crc32c.so instead of the package's (with --unchanged: a build of the parent commit)"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--shapes", default="1k,100k,ref")
ap.add_argument("--unchanged", action="store_true")
ap.add_argument("--lib", default=None)
args = ap.parse_args()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kvsep  # noqa: E402

if args.lib:  # another build of the library: it may predate the write-side entry points, which --unchanged does not call
    kvsep.LIB_PATH = os.path.abspath(args.lib)
    for new in ("kvsep_log_frame_layout", "kvsep_log_frame_device"):
        kvsep._SIGS.pop(new, None)

dev = torch.device("cuda:0")
i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device=dev)  # noqa: E731
u8 = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)  # noqa: E731


def timed(forms, rounds):
    times = {k: [] for k in forms}
    for r in range(rounds):
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            forms[k]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def report(row, times):
    for k, t in times.items():
        row[k + "_us"] = round(statistics.median(t), 1)
        row[k + "_runs_us"] = [round(x, 1) for x in t]
    print(json.dumps(row), flush=True)


def shapes():
    want = args.shapes.split(",")
    if "1k" in want:
        yield "65,536 records of 1 KiB", [1024] * 65536, 7
    if "100k" in want:
        yield "655 records of 100 KiB", [100 << 10] * 655, 8
    path = os.path.join(HERE, "..", "..", "tests", "golden", "ref_framing.json")
    if "ref" in want and os.path.exists(path):
        with open(path) as f:
            lg = json.load(f)["log"]
        yield "the 12 reference records", lg["lens"], lg["seed"]


ctx = kvsep.Context(0)
for name, lens, seed in shapes():
    lens = np.array(lens, np.uint64)
    count, total = lens.size, int(lens.sum())
    data = kvsep.splitmix64_bytes(total + 1, seed, 0)[:total]
    d = torch.from_numpy(data.copy()).to(dev)
    h_off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    d_off, d_len = torch.from_numpy(h_off.view(np.int64)).to(dev), torch.from_numpy(lens.view(np.int64)).to(dev)

    if args.unchanged:  # the two forms that share the copy kernel's template with the log frame
        first = torch.arange(count + 1, dtype=torch.int64, device=dev)
        at = torch.from_numpy((h_off + 8 * np.arange(count, dtype=np.uint64)).view(np.int64)).to(dev)
        dst, seg_crc, crc = u8(total + 8 * count), i32(count), i32(count)
        forms = {"pack": lambda: ctx.pack_device(d.data_ptr(), d_off, d_len, first, dst, total + 8 * count, at),
                 "vlog_frame": lambda: ctx.vlog_frame_device(d.data_ptr(), d_off, d_len, first, seg_crc, crc, dst,
                                                             total + 8 * count, at, total_bytes=total)}
        for f in forms.values():
            f()
            torch.cuda.synchronize()
        report({"shape": name, "lib": args.lib or "this build"}, timed(forms, args.rounds))
        continue

    _, _, nfrag, written = kvsep.log_frame_layout(lens)
    ctx.reserve(max(count, nfrag), total)
    rec_at, frag_first = i64(count), i64(count + 1)
    frag_off, frag_len, frag_at, frag_type, frag_crc = i64(nfrag), i64(nfrag), i64(nfrag), u8(nfrag), i32(nfrag)
    words = i64(4)
    dst, dst_host, dst_copy, crc2 = u8(written), u8(written), u8(written), i32(nfrag)
    seg_first = torch.arange(nfrag + 1, dtype=torch.int64, device=dev)
    pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
    image = np.zeros(written, np.uint8)
    addrs = np.uint64(pinned.data_ptr()) + h_off

    def frame_form(cap=nfrag, nbytes=written):
        ctx.log_frame_device(d.data_ptr(), d_off, d_len, 0, dst, nbytes, rec_at, frag_first, frag_off, frag_len, frag_at,
                             frag_type, frag_crc, words[0:1], words[1:2], count=count, frag_cap=cap, total_bytes=total)

    def host_form():
        pinned.copy_(d)
        torch.cuda.synchronize()
        ctx.frame_raw("log", addrs, lens, image, 0)
        dst_host.copy_(torch.from_numpy(image))

    forms = {"frame": frame_form, "host": host_form, "layout": lambda: frame_form(0, 0),
             "crc": lambda: ctx.batch_device(d.data_ptr(), frag_off, frag_len, crc2, count=nfrag, total_bytes=total,
                                             max_len=32761),
             "copy": lambda: ctx.pack_device(d.data_ptr(), frag_off, frag_len, seg_first, dst_copy, written, frag_at,
                                             count=nfrag, nseg=nfrag)}
    for f in forms.values():  # warm
        f()
        torch.cuda.synchronize()
    frame_form()
    torch.cuda.synchronize()
    same = bool(torch.equal(dst, dst_host)) and int(words[1].item()) == written
    report({"shape": name, "records": count, "bytes": total, "fragments": nfrag, "written": written, "same": same},
           timed(forms, args.rounds))

if not args.unchanged:
    for count in (65536, 1048576):  # the serial piece alone: lengths only
        d_len = torch.full((count,), 1024, dtype=torch.int64, device=dev)
        d_off = torch.arange(count, dtype=torch.int64, device=dev) * 1024
        rec_at, frag_first, words, one = i64(count), i64(count + 1), i64(4), u8(8)
        ctx.reserve(count, 0)

        def layout_form():
            ctx.log_frame_device(one.data_ptr(), d_off, d_len, 0, one, 0, rec_at, frag_first, None, None, None, None,
                                 None, words[0:1], words[1:2], count=count, frag_cap=0, total_bytes=0)

        layout_form()
        torch.cuda.synchronize()
        report({"shape": f"layout alone, {count} records of 1 KiB", "fragments": int(words[0].item())},
               timed({"layout": layout_form}, args.rounds))
ctx.close()
