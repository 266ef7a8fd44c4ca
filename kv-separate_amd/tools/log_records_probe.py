#!/usr/bin/env python3
"""What assembling the records of a device-resident log / MANIFEST image costs: kvsep_log_records_device against the
route such an image had without it.

Per image four forms, interleaved over the rounds in one process, each timed with an event pair on the stream (the host
steps of the last form lie between the events, so the pair spans them), medians and runs reported:
  records  kvsep_log_records_device: walk, checksum, accept rule, chains, layout and copy on the stream, no host step
  read     kvsep_log_read_device alone (the composite's first part)
  chains   kvsep_log_chains_device alone, on the arrays the read left (the part this probe is about)
  host     the route without the chains pass: log_read_device, a synchronise, D2H of off / len / type / accept / gap,
           the host assembly (kvsep_log_chains and a prefix sum in numpy) building first[] / dst_off[] and the
           fragment descriptors, H2D of them, pack_device
Images:
  1k      64 MiB of 1 KiB records (every record a FULL)
  100k    64 MiB of 100 KiB records (four fragments each)
  corpus  the base image of the recorded log corpus (tests/golden), when the file is there
The destination bytes of `records` and `host` are compared once.
usage: log_records_probe.py [--rounds 9] [--images 1k,100k,corpus] [--only-read] [--lib PATH]
  --only-read   time log_read_device alone (one JSON line an image): for A/B runs against another build of the library
  --lib PATH    load that libkvsep_crc32c.so instead of the package's (with --only-read: a build of the parent commit)"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--images", default="1k,100k,corpus")
ap.add_argument("--only-read", action="store_true")
ap.add_argument("--lib", default=None)
args = ap.parse_args()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kvsep  # noqa: E402

if args.lib:  # another build of the library: it may predate the assembly entry points, which --only-read does not call
    kvsep.LIB_PATH = os.path.abspath(args.lib)
    for new in ("kvsep_log_chains", "kvsep_log_chains_device", "kvsep_log_records_device"):
        kvsep._SIGS.pop(new, None)

dev = torch.device("cuda:0")


def framed(ctx, payloads):
    import ctypes
    lens = np.array([len(p) for p in payloads], np.uint64)
    bufs = [ctypes.create_string_buffer(p, len(p)) for p in payloads]
    ptrs = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
    cap = int(lens.sum()) + 7 * (len(payloads) + int(lens.sum()) // 32768 * 2 + 8) + 65536
    dst = np.zeros(cap, np.uint8)
    written = ctypes.c_uint64()
    rc = kvsep.lib().kvsep_log_frame_host(ctx._h, ptrs, lens.ctypes.data_as(ctypes.c_void_p), len(bufs), 0,
                                          dst.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(written))
    assert rc == 0, kvsep.lib().kvsep_last_error()
    return dst[:written.value].tobytes()


def images(ctx):
    want = args.images.split(",")
    rng = np.random.default_rng(7)
    if "1k" in want:
        body = rng.integers(0, 256, 1024, dtype=np.uint8).tobytes()
        yield "64 MiB of 1 KiB records", framed(ctx, [body] * 65024)[:64 << 20]
    if "100k" in want:
        body = rng.integers(0, 256, 100 << 10, dtype=np.uint8).tobytes()
        yield "64 MiB of 100 KiB records", framed(ctx, [body] * 655)[:64 << 20]
    path = os.path.join(HERE, "..", "..", "tests", "golden", "framing_corpus_log.json")
    if "corpus" in want and os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
        with open(os.path.join(os.path.dirname(path), doc["base"]), "rb") as f:
            yield "corpus base image", f.read()


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


ctx = kvsep.Context(0)
for name, img in images(ctx):
    n = len(img)
    d = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(dev)
    nrec = kvsep.log_walk(img)[0].size
    cap = nrec + 8
    ctx.reserve(max(cap, (n + 32767) // 32768), n)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)  # noqa: E731
    off, ln, stored, ty, ok, acc, gap = (i64(cap), i64(cap), torch.zeros(cap, dtype=torch.int32, device=dev), u8(cap),
                                         u8(cap), u8(cap), u8(cap))
    words = i64(8)  # nrec, dropped, bad_length, nchain, nwhole, end

    def read_form():
        ctx.log_read_device(d.data_ptr(), n, off, ln, stored, ty, ok, acc, words[0:1], gap=gap, dropped=words[1:2],
                            bad_length=words[2:3], cap=cap)

    if args.only_read:
        read_form()
        torch.cuda.synchronize()
        t = timed({"read": read_form}, args.rounds)["read"]
        print(json.dumps({"image": name, "lib": args.lib or "this build", "read_us": round(statistics.median(t), 1),
                          "read_runs_us": [round(x, 1) for x in t]}), flush=True)
        continue

    frag_off, frag_len, first, whole, rec_off, rec_len = i64(cap), i64(cap), i64(cap + 1), u8(cap), i64(cap), i64(cap)
    dst, dst_host = u8(n), u8(n)

    def records_form():
        ctx.log_records_device(d.data_ptr(), n, off, ln, stored, ty, ok, acc, gap, words[0:1], frag_off, frag_len,
                               first, whole, words[3:4], dst, n, rec_off, words[5:6], rec_len=rec_len,
                               nwhole=words[4:5], dropped=words[1:2], bad_length=words[2:3], cap=cap)

    def chains_form():
        ctx.log_chains_device(ty, acc, words[0:1], first, whole, words[3:4], gap=gap, off=off, length=ln,
                              frag_off=frag_off, frag_len=frag_len, nwhole=words[4:5], cap=cap)

    def host_form():
        read_form()
        torch.cuda.synchronize()
        k = min(int(words[0].item()), cap)
        h_off, h_len = off[:k].cpu().numpy().view(np.uint64), ln[:k].cpu().numpy().view(np.uint64)
        h_ty, h_acc, h_gap = ty[:k].cpu().numpy(), acc[:k].cpu().numpy(), gap[:k].cpu().numpy()
        f, w, nchain, _ = kvsep.log_chains(h_ty, h_acc, h_gap)
        size = np.add.reduceat(np.append(h_len - 1, np.uint64(0)), f[:nchain].astype(np.int64))[:nchain] if nchain else \
            np.zeros(0, np.uint64)
        size = np.where(w[:nchain] != 0, size, 0).astype(np.uint64)
        at = np.concatenate(([0], np.cumsum(size)[:-1])).astype(np.uint64) if nchain else size
        at = np.where(w[:nchain] != 0, at, np.uint64(0xFFFFFFFFFFFFFFFF))
        d_so = torch.from_numpy((h_off + 1).view(np.int64)).to(dev)
        d_sl = torch.from_numpy((h_len - 1).view(np.int64)).to(dev)
        d_f = torch.from_numpy(f[:nchain + 1].view(np.int64)).to(dev)
        d_at = torch.from_numpy(at.view(np.int64)).to(dev)
        ctx.pack_device(d.data_ptr(), d_so, d_sl, d_f, dst_host, n, d_at, count=nchain, nseg=k)

    forms = {"records": records_form, "read": read_form, "chains": chains_form, "host": host_form}
    for f in forms.values():  # warm
        f()
        torch.cuda.synchronize()
    end = int(words[5].item())
    same = bool(torch.equal(dst[:end], dst_host[:end])) and end > 0
    times = timed(forms, args.rounds)
    row = {"image": name, "bytes": n, "records": nrec, "logical": int(words[4].item()), "out_bytes": end, "same": same}
    for k in forms:
        row[k + "_us"] = round(statistics.median(times[k]), 1)
        row[k + "_runs_us"] = [round(t, 1) for t in times[k]]
    print(json.dumps(row), flush=True)
ctx.close()
