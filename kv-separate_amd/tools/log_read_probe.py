#!/usr/bin/env python3
"""What reading a device-resident log / MANIFEST image costs: kvsep_log_read_device against the host-walk route.

Per image two forms, interleaved over the rounds in one process, each timed with an event pair on the stream (the host
steps of the second form lie between the events, so the pair spans them), medians and runs reported:
  device  kvsep_log_read_device: walk, checksum and accept rule on the stream, no host step
  host    the route without it: D2H of the image, host kvsep_log_walk, H2D of off / len / stored,
          kvsep_log_verify_device, D2H of ok, host kvsep_log_accept_gaps
Images:
  64m     64 MiB of 1 KiB records, intact (log::Writer's framing through kvsep_log_frame_host)
  corpus  the base image of the recorded log corpus (tests/golden), when the file is there
  empty   one block of 4,681 empty records: a block-long chain of dependent header loads on one lane
Both forms' accept / gap / byte counts are compared once.
usage: log_read_probe.py [--rounds 9] [--images 64m,corpus,empty]"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kvsep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--images", default="64m,corpus,empty")
args = ap.parse_args()
dev = torch.device("cuda:0")


def framed(ctx, payloads):
    lens = np.array([len(p) for p in payloads], np.uint64)
    bufs = [ctypes.create_string_buffer(p, len(p)) for p in payloads]
    ptrs = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
    cap = int(lens.sum()) + 16 * len(payloads) + 65536
    dst = np.zeros(cap, np.uint8)
    written = ctypes.c_uint64()
    rc = kvsep.lib().kvsep_log_frame_host(ctx._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p), len(bufs), 0,
                                          dst.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(written))
    assert rc == 0, kvsep.lib().kvsep_last_error()
    return dst[:written.value].tobytes()


def images(ctx):
    want = args.images.split(",")
    if "64m" in want:
        body = np.random.default_rng(7).integers(0, 256, 1024, dtype=np.uint8).tobytes()
        yield "64 MiB of 1 KiB records", framed(ctx, [body] * 65024)[:64 << 20]
    path = os.path.join(HERE, "..", "..", "tests", "golden", "framing_corpus_log.json")
    if "corpus" in want and os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
        with open(os.path.join(os.path.dirname(path), doc["base"]), "rb") as f:
            yield "corpus base image", f.read()
    if "empty" in want:
        crc = kvsep.mask(kvsep.value(b"\x01"))
        yield "4,681 empty records", struct.pack("<IHB", crc, 0, 1) * 4681 + b"\0"


ctx = kvsep.Context(0)
for name, img in images(ctx):
    n = len(img)
    d = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(dev)
    nrec = kvsep.log_walk(img)[0].size
    cap = nrec + 8
    ctx.reserve(max(cap, (n + 32767) // 32768), n)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)  # noqa: E731
    off, ln, stored, ty, ok, acc, gap, words = (i64(cap), i64(cap), torch.zeros(cap, dtype=torch.int32, device=dev),
                                                u8(cap), u8(cap), u8(cap), u8(cap), i64(3))
    h_img = torch.empty(n, dtype=torch.uint8).pin_memory()
    result = {}

    def device_form():
        ctx.log_read_device(d.data_ptr(), n, off, ln, stored, ty, ok, acc, words[0:1], gap=gap, dropped=words[1:2],
                            bad_length=words[2:3], cap=cap)
        result["device"] = None

    def host_form():
        h_img.copy_(d)  # D2H, blocking
        o, l, s, _ = kvsep.log_walk(h_img.numpy())
        d_o = torch.from_numpy(o.view(np.int64)).to(dev)
        d_l = torch.from_numpy(l.view(np.int64)).to(dev)
        d_s = torch.from_numpy(s.view(np.int32)).to(dev)
        d_ok = torch.empty(o.size, dtype=torch.uint8, device=dev)
        ctx.log_verify_device(d.data_ptr(), d_o, d_l, d_s, d_ok, count=o.size, total_bytes=n, max_len=32762)
        result["host"] = kvsep.log_accept_gaps(h_img.numpy(), d_ok.cpu().numpy())

    forms = {"device": device_form, "host": host_form}
    for f in forms.values():  # warm
        f()
        torch.cuda.synchronize()
    a, g, dropped, bad = result["host"]
    same = bool(np.array_equal(acc.cpu().numpy()[:nrec], a) and np.array_equal(gap.cpu().numpy()[:nrec], g) and
                words.cpu().tolist() == [nrec, dropped, bad])
    times = {k: [] for k in forms}
    for r in range(args.rounds):
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            forms[k]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    row = {"image": name, "bytes": n, "records": nrec, "same": same}
    for k in forms:
        row[k + "_us"] = round(statistics.median(times[k]), 1)
        row[k + "_runs_us"] = [round(t, 1) for t in times[k]]
    print(json.dumps(row), flush=True)
ctx.close()
