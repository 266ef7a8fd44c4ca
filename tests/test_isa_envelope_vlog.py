"""The memory envelope of the value-log reader's kernels: the shipped gfx950 assembly reads and writes exactly what
crc32c_vlogwalk.inc and the public header promise.  CPU only.

tests/test_isa_envelope_framing.py does this for the framing, layout and log kernels; this file runs, under
tools/wave_emu.py and with that file's Call (one call's emulated memory and its checks),

  crc32c_vlogwalk.inc   vlog_walk / vlog_totals

with the shipped window (csrc/vlog_run.h), one workgroup of one wavefront each.  Per run:

 a. reads: the image's declared region is exactly the naturally aligned 16-byte granules that hold a byte of
    [base, base + n): it begins at the granule of the first byte and ends with the granule of the last, with nothing
    mapped around it, so a load outside the envelope is the emulator's "bad address".  With base on a granule boundary
    the image starts on the first byte of its region, with base + n on one it ends on the last.  An empty image has a
    base that is mapped nowhere.  The totals kernel's off / len are regions of exactly min(*nrec, cap) elements;
 b. writes: the image carries no write mark; off / len / stored carry one on every byte of their cap elements, *nrec
    and *consumed on every byte; the totals kernel writes its five words and nothing else;
 c. results: equal to kvsep.vlog_walk and to the totals rule restated here;
 d. cost: the wave-instructions of each case are printed (pytest -s shows them).
"""
import os
import re
import struct

import numpy as np
import pytest

import test_isa_envelope_framing as F

env = F.env  # the module fixture that builds the assembly and loads the emulator
CSRC, ASM, M64, FAR = F.CSRC, F.ASM, F.M64, F.FAR

K = {"vlog_walk": "_ZN5kvsep16vlog_walk_kernelENS_12VlogWalkArgsE",
     "vlog_totals": "_ZN5kvsep18vlog_totals_kernelENS_14VlogTotalsArgsE"}
STRUCTS = {"VlogWalkArgs": "crc32c_vlogwalk.inc", "VlogTotalsArgs": "crc32c_vlogwalk.inc"}
HEADER = open(os.path.join(CSRC, "vlog_run.h")).read()
WINDOW = int(re.search(r"#define KVSEP_VLOG_WINDOW (\d+)", HEADER).group(1))
LANES = int(re.search(r"constexpr uint32_t kLanes = (\d+);", HEADER).group(1))
PAD_STORED = int(re.search(r"constexpr uint32_t kPadStored = (0x[0-9a-f]+)u;", HEADER).group(1), 16)


class Call(F.Call):
    """F.Call with this file's kernel names and structs, and the image in a region of exactly its granules."""

    def launch(self, kernel, args):
        try:
            self.steps += self.E.launch_args(self.mem, ASM, K[kernel], LANES, args, 1)
        except self.E.EmuError as e:
            raise AssertionError("%s: %s: %s\n  arrays: %s" % (
                self.tag, kernel, e, ", ".join("%s@0x%x+%d" % (n, a, self.size[n]) for n, a in self.addr.items()))) from e

    def sargs(self, kernel, struct_name, values):
        return self.E.struct_kernarg(ASM, K[kernel], os.path.join(CSRC, STRUCTS[struct_name]), struct_name, values)

    def granules(self, data, skew):
        """The image with its first byte `skew` past a 16-byte boundary, in a region that is its granules and no more."""
        data = np.ascontiguousarray(data, np.uint8)
        if not data.size:
            return FAR
        size = -(-(skew + data.size) // 16) * 16
        fill = np.full(size, 0xEE, np.uint8)
        fill[skew:skew + data.size] = data
        region = self.mem.alloc(size, align=4096, data=fill, phase=4096 - size % 4096 if size % 4096 else 0)
        assert region % 16 == 0 and (region + size) % 4096 == 0  # the region ends on a page's last byte
        self.kind[region] = ("in", "image")
        self.addr["image"], self.size["image"] = region, size
        return region + skew


def frame(lengths, rng):
    out = bytearray()
    for l in lengths:
        out += rng.integers(0, 256, 4, dtype=np.uint8).tobytes() + struct.pack("<I", l) + \
            rng.integers(0, 256, l, dtype=np.uint8).tobytes()
    return out


def run(env, tag, img, skew, cap_delta, first_bad=None):
    """vlog_walk_kernel over the image, then vlog_totals_kernel over its arrays with the verdict words the test gives
    (first_bad: None for a clean batch, else a record's index)."""
    from kvsep import vlog_walk
    img = np.frombuffer(bytes(img), np.uint8)
    n = img.size
    off, ln, st, consumed = vlog_walk(img)
    nrec = off.size
    cap = max(nrec + cap_delta, 0)
    held = min(nrec, cap)
    c = Call(env, tag)
    d_img = c.granules(img, skew)
    v = dict(img=d_img, n=n, off=c.output("off", 8 * cap), len=c.output("len", 8 * cap),
             stored=c.output("stored", 4 * cap), cap=cap, nrec=c.output("nrec", 8), consumed=c.output("consumed", 8))
    c.launch("vlog_walk", c.sargs("vlog_walk", "VlogWalkArgs", v))
    assert int(c.get("nrec", np.uint64)[0]) == nrec, "%s: *nrec %d, the host walk finds %d" % (
        tag, int(c.get("nrec", np.uint64)[0]), nrec)
    assert int(c.get("consumed", np.uint64)[0]) == consumed, tag
    for name, ref, dt, pad in (("off", off, np.uint64, 0), ("len", ln, np.uint64, 0), ("stored", st, np.uint32, PAD_STORED)):
        exp = np.full(cap, pad, dt)
        exp[:held] = ref[:held]
        got = c.get(name, dt)
        assert np.array_equal(got, exp), "%s: %s differs at %s" % (tag, name, np.nonzero(got != exp)[0][:8])
    c.check()  # the image is an input: never written; every output byte written
    walk_steps = c.steps

    # ---- the totals: off / len are arrays of exactly `held` elements
    t = Call(env, tag + " totals")
    fb = M64 if first_bad is None or first_bad >= held else first_bad
    tv = dict(first_bad_in=t.input("first_bad_in", np.array([fb], np.uint64)),
              nbad_in=t.input("nbad_in", np.array([0 if fb == M64 else 1], np.uint64)),
              nrec=t.input("nrec", np.array([nrec], np.uint64)), off=t.input("off", off[:held]),
              len=t.input("len", ln[:held]), cap=cap, first_bad=t.output("first_bad", 8), nbad=t.output("nbad", 8),
              ngood=t.output("ngood", 8), good_bytes=t.output("good_bytes", 8), drop_bytes=t.output("drop_bytes", 8))
    t.launch("vlog_totals", t.sargs("vlog_totals", "VlogTotalsArgs", tv))
    g = held if fb == M64 else fb
    want = (fb, 0 if fb == M64 else 1, g, int(off[g - 1] + ln[g - 1]) if g else 0, int(ln[g]) if g < held else 0)
    got = tuple(int(t.get(k, np.uint64)[0]) for k in ("first_bad", "nbad", "ngood", "good_bytes", "drop_bytes"))
    assert got == want, "%s: totals %s, expected %s" % (tag, got, want)
    t.steps += walk_steps
    t.check()


def cases():
    rng = np.random.default_rng(14)
    out = [("empty image", b"", 0, 3, None),
           ("7 bytes: no header", bytes(7), 1, 2, None),
           ("one empty record, starts on its region's first byte", frame([0], rng), 0, 0, 0),
           ("a length word of 0xFFFFFFFF in a 20-byte image", bytes([1, 2, 3, 4, 255, 255, 255, 255]) + bytes(12), 9, 1, None)]
    img = frame([5, 0, 40, 11], rng)  # 88 bytes: base + n on a granule boundary at skew 8
    assert (8 + len(img)) % 16 == 0
    out.append(("ends on its region's last byte", img, 8, 0, 2))
    img = frame([8, 0, 24, 100, 4], rng)
    assert len(img) % 16 == 0
    out.append(("starts on the first and ends on the last byte of its region", img, 0, -1, None))
    for delta, skew in ((-9, 0), (-8, 15), (-7, 15), (-1, 0), (0, 3), (1, 0)):
        # the second header WINDOW + delta bytes past the first granule's start; then records into a third window
        q = WINDOW - skew + delta
        img = frame([q - 8, 20, 3, WINDOW, 1], rng) + bytes([0xF1] * 5)
        out.append(("second header at window end %+d skew %d" % (delta, skew), img, skew, 2, 3))
    out.append(("130 small records, arrays cut", frame([i % 5 for i in range(130)], rng), 5, -2, 64))
    out.append(("129 empty records, padding", frame([0] * 129, rng), 15, 70, None))
    return out


CASES = cases()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c[0] for c in CASES])
def test_vlog_read(env, ci):
    tag, img, skew, cap_delta, first_bad = CASES[ci]
    run(env, "vlog " + tag, img, skew, cap_delta, first_bad)
