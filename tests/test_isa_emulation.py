"""Functional emulation of the shipped CRC kernels' gfx950 assembly.  CPU only.

tools/wave_emu.py executes the compiled .s (the --save-temps output `make -C kv-separate_amd asm` keeps under build/)
instruction by instruction -- 64-lane VGPRs under EXEC, SGPRs, LDS, scalar / vector memory, ds_bpermute and DPP --
for one workgroup of the real 256-workgroup grid, and the CRCs it writes are compared with the oracle.  Round 3's
sorted-window fault was a code-generation error of exactly this kind (a rematerialised table base restored under the
narrowed EXEC of a nested divergent branch, so the slot-end lanes of every later group read the wrong table); the
emulator reproduced it from the diag build's assembly (tools/sorted_vin_emulate.py, retired in round 6: commit 8853f41) and
this test runs the same check
on every shipped narrow-family kernel, plain and verify forms, so a miscompile of that class fails on the CPU.  The
wide kernel runs too: unplanned (static runs, one workgroup of the grid) and planned (host-built piece table exactly
as the plan kernels build it, the guided schedule, then every workgroup of the combine kernel).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kv-separate_amd")
ASM = os.path.join(PKG, "build", "crc32c_device-hip-amdgcn-amd-amdhsa-gfx950.s")
sys.path.insert(0, os.path.join(PKG, "tools"))
sys.path.insert(0, PKG)

# the shipped narrow-family templates (launch_narrow_v in csrc/crc32c_device.hip): name, threads per workgroup.  The
# claim kernel's waves take groups through an LDS counter; the emulator runs a workgroup's waves to each barrier in
# order, so its deal differs from the hardware's (a different interleaving, the same set of groups)
SORTED = "_ZN5kvsep27crc32c_narrow_sorted_kernelILi4ELb1ELi1024ELb%dENS_5ExactEEEvNS_10PiecesArgsE"
NARROW16 = "_ZN5kvsep20crc32c_narrow_kernelILi4ELb1ELi1024ELb0ELb1ENS_7LdsFullELb%dENS_5ExactEEEvNS_10PiecesArgsE"
NARROW8 = "_ZN5kvsep20crc32c_narrow_kernelILi4ELb1ELi512ELb1ELb1ENS_7LdsFullELb%dENS_5ExactEEEvNS_10PiecesArgsE"
CLAIM = "_ZN5kvsep26crc32c_narrow_claim_kernelILi4ELi512ELb%dELb1ELi8ELj3EEEvNS_10PiecesArgsE"  # kLean 3 (round 6)
CLAIM16 = "_ZN5kvsep26crc32c_narrow_claim_kernelILi4ELi512ELb%dELb1ELi16ELj0EEEvNS_10PiecesArgsE"
# the cooperative kernel (round 6, narrow form 12): the workgroup's 8 waves on one group, one barrier per group;
# init-less template (kInit false: no init word loaded)
COOP = "_ZN5kvsep25crc32c_narrow_coop_kernelILb%dELb0EEEvNS_10PiecesArgsE"
# (label, template, threads per workgroup, arrival levels of the verify publish: 8 = per-XCD shards, then the final word)
KERNELS = [("sorted", SORTED, 1024, 1), ("narrow16", NARROW16, 1024, 1), ("narrow8", NARROW8, 512, 1),
           ("claim", CLAIM, 512, 8), ("claim16", CLAIM16, 512, 8), ("coop", COOP, 512, 8)]


@pytest.fixture(scope="module")
def env():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-s", "-C", PKG, "asm"], stdout=subprocess.DEVNULL)
    import wave_emu
    from kvsep import mask, splitmix64_bytes
    return wave_emu, wave_emu.dev_tables(), mask, splitmix64_bytes


def batch(kind, splitmix64_bytes):
    rng = np.random.default_rng(7)
    if kind == "short":  # the sorted-window probe's shape: 0..39 B, hint = max
        n, ln = 20000, rng.integers(0, 40, 20000)
        hint = 39
    else:  # up to 600 B with an understated hint of 256: the deferred-block path (narrow_deferred) runs too
        n, ln = 12000, rng.integers(0, 601, 12000)
        hint = 256
    ln = ln.astype(np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    off += np.uint64(3)  # unaligned starts
    data = splitmix64_bytes(int(off[-1] + ln[-1]) + 4096, 11, 0)
    return data, off, ln, hint


@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("label,tmpl,threads,shards", KERNELS)
def test_emulated_kernel_matches_oracle(env, label, tmpl, threads, shards, kind):
    E, tabs, mask, splitmix64_bytes = env
    data, off, ln, hint = batch(kind, splitmix64_bytes)
    exp = load_oracle().batch(data, off, ln, None, threads=8)
    wg = 5
    out, written, _, _, _ = E.run_batch_kernel(ASM, tmpl % 0, threads, data, off, ln, tabs, wg=wg, hint=hint)
    mine = np.nonzero(written)[0]
    assert mine.size > 0, "workgroup wrote nothing"
    assert np.array_equal(out[mine], exp[mine]), f"{label}: {np.count_nonzero(out[mine] != exp[mine])} wrong CRCs"
    if kind == "long":
        assert ln[mine].max() > hint, "the deferred path was not exercised"
    # verify form: the same workgroup with three wrong stored words among its blocks
    stored = np.array([mask(int(x)) for x in exp], np.uint32)
    plant = mine[[0, mine.size // 2, mine.size - 1]]
    stored[plant] ^= 0x100
    out_v, written_v, fb, nb, _ = E.run_batch_kernel(ASM, tmpl % 1, threads, data, off, ln, tabs, wg=wg, hint=hint,
                                                    expect=stored, shards=shards)
    assert np.array_equal(np.nonzero(written_v)[0], mine)
    assert np.array_equal(out_v[mine], exp[mine])
    assert (fb, nb) == (int(plant.min()), 3)  # published by this (last) workgroup, accumulators reset (batch_results)
    if kind == "short":  # every block of the workgroup bad: every wave's verdict, several mismatches per wave
        bad = np.array([mask(int(x)) for x in exp], np.uint32) ^ np.uint32(0x100)
        *_, fb, nb, _ = E.run_batch_kernel(ASM, tmpl % 1, threads, data, off, ln, tabs, wg=wg, hint=hint, expect=bad,
                                           shards=shards)
        assert (fb, nb) == (int(mine.min()), int(mine.size))
    _verify_tail(E, tmpl % 1, threads, data, off, ln, tabs, wg, hint, exp, mask, mine, plant, shards=shards)
    # the captured form (round 6): the workgroup's verdict in its own slot, nothing published, no accumulator touched
    st = {}
    out_s, written_s, fb, nb, _ = E.run_batch_kernel(ASM, tmpl % 1, threads, data, off, ln, tabs, wg=wg, hint=hint,
                                                     expect=stored, shards=shards, vslot=True, state=st)
    assert np.array_equal(np.nonzero(written_s)[0], mine) and np.array_equal(out_s[mine], exp[mine])
    assert (fb, nb) == (E.SENTINEL, E.SENTINEL)
    sl = st["slots"]
    assert sl[wg] == (int(plant.min()), 3), sl[wg]
    assert all(v == (E.SENTINEL, E.SENTINEL) for i, v in enumerate(sl) if i != wg)


def _verify_tail(E, name, threads, data, off, ln, tabs, wg, hint, exp, mask, mine, plant, lds_bytes=160768, shards=1):
    """The verify form's end (verify_publish): a clean batch publishes (-1, 0) from the last workgroup; a workgroup that
    is not the last leaves the caller's words alone and its posts -- lowest index, count, one arrival -- in the
    accumulators for the last one."""
    clean = np.array([mask(int(x)) for x in exp], np.uint32)
    *_, fb, nb, _ = E.run_batch_kernel(ASM, name, threads, data, off, ln, tabs, wg=wg, hint=hint, expect=clean,
                                       lds_bytes=lds_bytes, shards=shards)
    assert (fb, nb) == (-1, 0)
    stored = clean.copy()
    stored[plant] ^= 0x100
    st = {}
    *_, fb, nb, _ = E.run_batch_kernel(ASM, name, threads, data, off, ln, tabs, wg=wg, hint=hint, expect=stored,
                                       lds_bytes=lds_bytes, last=False, state=st, shards=shards)
    assert (fb, nb) == (E.SENTINEL, E.SENTINEL)  # not published
    # the workgroup's count travels with its arrival (round 5): on the final word (one level) or on the workgroup's
    # shard word (two levels); its lowest bad block on vacc[0]
    sh = [0] * E.VACC_SHARDS
    if shards > 1:
        sh[wg % shards] = (1 << 40) | len(plant)
    final = (len(plant) | (1 << 40)) if shards == 1 else 0
    assert st["vacc"] == (int(plant.min()), final, *sh), [hex(v) for v in st["vacc"]]


PIECES = "_ZN5kvsep20crc32c_pieces_kernelILb%dELb%dELi4ELb1ELb1ELi512ELb1ELb%dENS_5ExactEEEvNS_10PiecesArgsE"
COMBINE = "_ZN5kvsep21crc32c_combine_kernelILb%dEEEvNS_10PiecesArgsE"


def _planted(exp, mask, idx):
    stored = np.array([mask(int(x)) for x in exp], np.uint32)
    stored[idx] ^= 0x100
    return stored


@pytest.mark.parametrize("verify", [0, 1])
def test_emulated_wide_unplanned(env, verify):
    """The wide kernel on an unsplit batch (static contiguous runs): one workgroup of the grid."""
    E, tabs, mask, splitmix64_bytes = env
    rng = np.random.default_rng(3)
    n = 4096
    ln = rng.integers(0, 5000, n).astype(np.uint64)
    ln[rng.integers(0, n, 64)] = rng.integers(0, 16, 64)  # head/tail-only blocks
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1] + np.uint64(5), dtype=np.uint64)  # 5-B gaps: every start alignment
    data = splitmix64_bytes(int(off[-1] + ln[-1]) + 4096, 13, 0)
    exp = load_oracle().batch(data, off, ln, None, threads=8)
    out, written, _, _, _ = E.run_batch_kernel(ASM, PIECES % (0, 0, 0), 512, data, off, ln, tabs, wg=7,
                                               lds_bytes=160768)
    mine = np.nonzero(written)[0]
    assert mine.size > 0 and np.array_equal(out[mine], exp[mine])
    # per-block initial CRCs: the padded head rewinds each block's register to its 16-B boundary (x^-8k)
    init = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    exp_i = load_oracle().batch(data, off, ln, init, threads=8)
    out_i, wi, _, _, _ = E.run_batch_kernel(ASM, PIECES % (0, 0, 0), 512, data, off, ln, tabs, wg=7, init=init)
    assert np.array_equal(np.nonzero(wi)[0], mine) and np.array_equal(out_i[mine], exp_i[mine])
    if verify:
        plant = mine[[0, mine.size - 1]]
        out_v, wv, fb, nb, _ = E.run_batch_kernel(ASM, PIECES % (0, 0, 1), 512, data, off, ln, tabs, wg=7,
                                                  expect=_planted(exp, mask, plant))
        assert np.array_equal(np.nonzero(wv)[0], mine) and np.array_equal(out_v[mine], exp[mine])
        assert (fb, nb) == (int(plant.min()), 2)
        _verify_tail(E, PIECES % (0, 0, 1), 512, data, off, ln, tabs, 7, 0, exp, mask, mine, plant)


@pytest.mark.parametrize("verify", [0, 1])
def test_emulated_wide_planned_with_combine(env, verify):
    """A split batch as the large configs run it: piece table, the wide kernel's guided schedule (one workgroup takes
    every item here), the combine kernel's Horner step over the pieces; 16 KiB pieces, blocks up to 100 KiB."""
    E, tabs, mask, splitmix64_bytes = env
    rng = np.random.default_rng(4)
    n = 40
    ln = rng.integers(0, 100 * 1024, n).astype(np.uint64)
    ln[:4] = [0, 1, 32 * 1024, 32 * 1024 - 1]  # empty, one byte, exactly 2P (split), just under 2P (not split)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1] + np.uint64(3), dtype=np.uint64)
    data = splitmix64_bytes(int(off[-1] + ln[-1]) + 4096, 17, 0)
    exp = load_oracle().batch(data, off, ln, None, threads=8)
    expect = None
    plant = np.array([2, 5, n - 1])  # a split block and two others
    if verify:
        expect = _planted(exp, mask, plant)
    out, written, fb, nb, _ = E.run_planned_batch(ASM, PIECES % (1, 1, verify), COMBINE % verify, data, off, ln, tabs,
                                                  expect=expect)
    assert written.all()
    assert np.array_equal(out, exp), f"{np.count_nonzero(out != exp)} wrong CRCs"
    if verify:
        assert (fb, nb) == (2, 3)  # the combine kernel's last workgroup published; accumulators reset (batch_results)
        # captured: the pieces kernel's workgroup 5 (the whole blocks) and the combine kernel's one workgroup (the
        # split ones) each write their slot, clean or not; the reduce kernel's min / sum over the slots is the verdict
        st = {}
        out_s, _, fb, nb, _ = E.run_planned_batch(ASM, PIECES % (1, 1, 1), COMBINE % 1, data, off, ln, tabs,
                                                  expect=expect, state=st)
        assert np.array_equal(out_s, exp) and (fb, nb) == (E.SENTINEL, E.SENTINEL)
        sl = st["slots"]
        split = set(np.nonzero(ln >= 2 * 16 * 1024)[0].tolist())
        whole = [int(b) for b in plant if int(b) not in split]
        assert sl[5] == ((min(whole), len(whole)) if whole else ((1 << 64) - 1, 0)), sl[5]
        assert sl[256] == (min(int(b) for b in plant if int(b) in split), len(plant) - len(whole)), sl[256]
        written = [v for v in sl if v != (E.SENTINEL, E.SENTINEL)]
        assert len(written) == 2 and min(v[0] for v in written) == 2 and sum(v[1] for v in written) == 3
        _, _, fb, nb, _ = E.run_planned_batch(ASM, PIECES % (1, 1, 1), COMBINE % 1, data, off, ln, tabs,
                                              expect=_planted(exp, mask, np.array([], np.int64)))
        assert (fb, nb) == (-1, 0)


# ------------------------------------------------------------------------------------------------------------------
# The opcodes the layout, log and list kernels add (tests/test_isa_envelope_framing.py): one instruction at a time
# against a plain Python integer definition, on edge operands, with every third lane masked off by EXEC -- an inactive
# lane keeps its destination, and writes 0 into a carry / compare mask.
M32 = 0xFFFFFFFF
EDGE32 = [0, 1, 2, 3, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, 0x7FFFFFFF,
          0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 0x12345678, 0x89ABCDEF, 0x00FF00FF, 31, 32, 63, 64]
EXEC = sum(1 << l for l in range(64) if l % 3 != 2)
KEPT = 0x5A5A5A5A  # what an inactive lane's destination holds before and after


class One:
    """A wave for single instructions: v1, v2, v3 hold edge operands in every pairing, v0 is the destination."""

    def __init__(self):
        import wave_emu as E
        self.E = E
        self.wg = E.Workgroup(E.Memory(), [], {}, 64, 65536, 0, 0)
        self.w = self.wg.waves[0]
        self.w.exec = EXEC

    def run(self, text):
        k = self.E.Insn(0, text)
        self.wg.exec_insn(self.w, k, k.op, k.ops)

    def lanes(self, *cols):
        for r, c in enumerate(cols, 1):
            self.w.v[r] = np.array(c, np.uint32)
        self.w.v[0] = np.full(64, KEPT, np.uint32)

    def check(self, text, want, a, b=None, c=None):
        """want(a, b, c) per active lane against v0 after `text`; the operand triples cover EDGE32 in rotation."""
        for rot_b in range(0, len(EDGE32), 5):
            for rot_c in ((0, 7) if c is not None else (0,)):
                A = [EDGE32[l % len(EDGE32)] for l in range(64)]
                B = [EDGE32[(l + rot_b) % len(EDGE32)] for l in range(64)]
                C = [EDGE32[(l * 3 + rot_c) % len(EDGE32)] for l in range(64)]
                self.lanes(A, B, C)
                self.run(text)
                for l in range(64):
                    exp = want(A[l], B[l], C[l]) & M32 if EXEC >> l & 1 else KEPT
                    assert int(self.w.v[0][l]) == exp, "%s lane %d: a=%#x b=%#x c=%#x -> %#x, want %#x" % (
                        text, l, A[l], B[l], C[l], int(self.w.v[0][l]), exp)


def _bitop3(imm, a, b, c):
    r = 0
    for i in range(8):
        if imm >> i & 1:
            r |= (a if i & 4 else ~a) & (b if i & 2 else ~b) & (c if i & 1 else ~c)
    return r & M32


VALU_CASES = [
    ("v_alignbyte_b32 v0, v1, v2, v3", lambda a, b, c: ((a << 32 | b) >> 8 * (c & 3))),
    ("v_add_u16_e32 v0, v1, v2", lambda a, b, c: (a + b) & 0xFFFF),
    ("v_or3_b32 v0, v1, v2, v3", lambda a, b, c: a | b | c),
    ("v_bitop3_b16 v0, v1, v2, v3 bitop3:0xc3", lambda a, b, c: (KEPT & 0xFFFF0000) | (_bitop3(0xC3, a, b, c) & 0xFFFF)),
    ("v_bitop3_b16 v0, v1, 1, v3 bitop3:0xc", lambda a, b, c: (KEPT & 0xFFFF0000) | (_bitop3(0xC, a, 1, c) & 0xFFFF)),
    ("v_mul_u32_u24_e32 v0, v1, v2", lambda a, b, c: (a & 0xFFFFFF) * (b & 0xFFFFFF)),
    ("v_mul_hi_u32_u24_e32 v0, v1, v2", lambda a, b, c: ((a & 0xFFFFFF) * (b & 0xFFFFFF)) >> 32),
    ("v_ffbh_u32_e32 v0, v1", lambda a, b, c: 32 - a.bit_length() if a else M32),
    ("v_ffbl_b32_e32 v0, v1", lambda a, b, c: (a & -a).bit_length() - 1 if a else M32),
    ("v_bcnt_u32_b32 v0, v1, v2", lambda a, b, c: bin(a).count("1") + b),
]


@pytest.mark.parametrize("text,want", VALU_CASES, ids=[t.split()[0] for t, _ in VALU_CASES])
def test_added_valu_opcode(text, want):
    One().check(text, want, True, True, True)


@pytest.mark.parametrize("text", ["v_subbrev_co_u32_e32 v0, vcc, v1, v2, vcc",
                                  "v_subbrev_co_u32_e64 v0, s[10:11], v1, v2, s[12:13]"])
def test_added_subbrev(text):
    """d = src1 - src0 - borrow in; borrow out per active lane, 0 for an inactive one.  Borrow in 0, all ones, mixed."""
    for cin in (0, (1 << 64) - 1, 0xF0F0F0F0AAAA5555):
        o = One()
        A = [EDGE32[l % len(EDGE32)] for l in range(64)]
        B = [EDGE32[(l * 7 + 3) % len(EDGE32)] for l in range(64)]
        B[:6] = A[:6]  # equal operands: the borrow in alone decides
        o.lanes(A, B)
        o.w.vcc = cin
        o.w.s[12], o.w.s[13] = cin & M32, cin >> 32
        o.run(text)
        out = o.w.vcc if "e32" in text else o.w.s[10] | o.w.s[11] << 32
        for l in range(64):
            act, ci = EXEC >> l & 1, cin >> l & 1
            r = B[l] - A[l] - ci
            assert int(o.w.v[0][l]) == (r & M32 if act else KEPT), (text, l, hex(cin))
            assert out >> l & 1 == (1 if act and r < 0 else 0), (text, l, hex(cin))


CMP_PY = {"eq": lambda a, b: a == b, "ne": lambda a, b: a != b, "lt": lambda a, b: a < b, "le": lambda a, b: a <= b,
          "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b}


@pytest.mark.parametrize("t", ["u16", "i16"])
@pytest.mark.parametrize("c", list(CMP_PY))
def test_added_compare16(c, t):
    """16-bit compares see the low halves only (as signed for i16); e32 writes VCC, e64 an SGPR pair."""
    def half(x):
        x &= 0xFFFF
        return x - 0x10000 if t == "i16" and x & 0x8000 else x
    for text, dst in (("v_cmp_%s_%s_e32 vcc, v1, v2" % (c, t), "vcc"), ("v_cmp_%s_%s_e64 s[20:21], v1, v2" % (c, t), "s")):
        o = One()
        A = [EDGE32[l % len(EDGE32)] for l in range(64)]
        B = [EDGE32[(l * 5 + 1) % len(EDGE32)] for l in range(64)]
        B[:8] = [x ^ 0xABCD0000 for x in A[:8]]  # equal low halves, different high halves
        o.lanes(A, B)
        o.run(text)
        out = o.w.vcc if dst == "vcc" else o.w.s[20] | o.w.s[21] << 32
        for l in range(64):
            assert out >> l & 1 == int(bool(EXEC >> l & 1) and CMP_PY[c](half(A[l]), half(B[l]))), (text, l)
    o = One()  # an inline constant operand
    o.lanes([0, 1, 0x10000, 0x1FFFF] * 16, [0] * 64)
    o.run("v_cmp_ne_u16_e32 vcc, 0, v1")
    assert o.w.vcc == sum(1 << l for l in range(64) if EXEC >> l & 1 and l % 4 in (1, 3))


def test_added_salu_opcodes():
    o = One()
    for v in [0, 1, 2, 0x80000000, M32, 0x00010000, 0x7FFFFFFF, 1 << 63, (1 << 64) - 1, 1 << 32, 0x0000FFFF00000000]:
        o.w.s[4], o.w.s[5] = v & M32, v >> 32
        o.run("s_flbit_i32_b64 s6, s[4:5]")
        assert o.w.s[6] == (64 - v.bit_length() if v else M32), hex(v)
        o.run("s_flbit_i32_b32 s6, s4")
        assert o.w.s[6] == (32 - (v & M32).bit_length() if v & M32 else M32), hex(v)
        o.run("s_brev_b32 s6, s4")
        assert o.w.s[6] == int("{:032b}".format(v & M32)[::-1], 2), hex(v)
        a, b = v & M32, 0x1234FFFF00FF00FF & M32
        o.w.s[7] = b
        o.w.s[8], o.w.s[9] = 0xFFFFFFFF, 0x0F0F0F0F
        o.run("s_nor_b64 s[10:11], s[4:5], s[8:9]")
        want = ~(v | 0x0F0F0F0FFFFFFFFF) & ((1 << 64) - 1)
        assert (o.w.s[10] | o.w.s[11] << 32, o.w.scc) == (want, int(want != 0)), hex(v)
    for a in (0, 1, 0x7FFF, 0x8000, 0xFFFF, 0x10000, M32):
        for imm in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
            o.w.s[4] = a
            o.run("s_cmpk_lt_u32 s4, 0x%x" % imm)
            assert o.w.scc == int(a < imm), (a, imm)  # the immediate zero-extends: 0x8000 is 32768
            o.run("s_cmpk_ge_u32 s4, 0x%x" % imm)
            assert o.w.scc == int(a >= imm), (a, imm)
            o.run("s_cmpk_lt_i32 s4, 0x%x" % imm)
            sa, si = a - (1 << 32) if a >> 31 else a, imm - 0x10000 if imm & 0x8000 else imm
            assert o.w.scc == int(sa < si), (a, imm)


def test_added_lds_pair_opcodes():
    """ds_read2 / ds_write2 (_b32, _b64; st64: offsets in units of 64 elements): two elements at addr + offset0 * size and
    addr + offset1 * size, against the single-element ops' view of the same LDS; inactive lanes neither store nor load."""
    for op, n, unit in (("2_b32", 1, 4), ("2_b64", 2, 8), ("2st64_b64", 2, 512), ("2st64_b32", 1, 256)):
        for o0, o1 in ((0, 1), (3, 255 if unit < 256 else 4), (61, 62) if unit < 256 else (1, 0)):
            o = One()
            # st64: a lane per element inside the first 64-element unit, so no two lanes' pairs overlap; else every lane
            # at address 0 (the last active lane's data stays)
            addr = np.arange(64, dtype=np.uint32) * np.uint32(4 * n if unit >= 256 else 0)
            o.w.v[1] = addr
            data = [np.arange(64, dtype=np.uint32) * np.uint32(0x01010101 * (r + 1)) + np.uint32(r << 28)
                    for r in range(4)]
            for r in range(4):
                o.w.v[4 + r] = data[r]
            regs = ("v4", "v5") if n == 1 else ("v[4:5]", "v[6:7]")
            o.run("ds_write%s v1, %s, %s offset0:%d offset1:%d" % (op, regs[0], regs[1], o0, o1))
            last = max(l for l in range(64) if EXEC >> l & 1)
            lds = o.wg.lds
            for e, off in enumerate((o0, o1)):
                for l in (range(64) if unit >= 256 else [last]):
                    at = int(addr[l]) + off * unit
                    got = [int.from_bytes(lds[at + 4 * i:at + 4 * i + 4].tobytes(), "little") for i in range(n)]
                    if unit >= 256 and not EXEC >> l & 1:
                        assert got == [0] * n, (op, l)  # an inactive lane stored nothing
                    else:
                        assert got == [int(data[e * n + i][l]) for i in range(n)], (op, o0, o1, l, e)
            for r in range(8, 12):
                o.w.v[r] = np.full(64, KEPT, np.uint32)
            dst = "v[8:9]" if n == 1 else "v[8:11]"
            o.run("ds_read%s %s, v1 offset0:%d offset1:%d" % (op, dst, o0, o1))
            for l in range(64):
                for e, off in enumerate((o0, o1)):
                    at = int(addr[l]) + off * unit
                    for i in range(n):
                        want = int.from_bytes(lds[at + 4 * i:at + 4 * i + 4].tobytes(), "little") if EXEC >> l & 1 \
                            else KEPT
                        assert int(o.w.v[8 + e * n + i][l]) == want, (op, o0, o1, l, e, i)


def test_added_byte_and_short_memory_opcodes():
    """global_load_ubyte / sbyte / ushort / sshort and global_store_byte / short: the addressed bytes only (marks on
    exactly those), zero- or sign-extended; inactive lanes touch nothing."""
    import wave_emu as E
    mem = E.Memory(track=True)
    src = np.arange(256, dtype=np.uint8) * np.uint8(37) + np.uint8(0x7D)
    base = mem.alloc(256, data=src)
    dstb = mem.alloc(256)
    wg = E.Workgroup(mem, [], {}, 64, 0, 0, 0)
    w = wg.waves[0]
    w.exec = EXEC

    def run(text):
        k = E.Insn(0, text)
        wg.exec_insn(w, k, k.op, k.ops)

    w.s[4], w.s[5] = base & M32, base >> 32
    w.s[6], w.s[7] = dstb & M32, dstb >> 32
    w.v[1] = np.arange(64, dtype=np.uint32) * np.uint32(3) + np.uint32(1)  # odd and even addresses
    for op, nb, signed in (("ubyte", 1, False), ("sbyte", 1, True), ("ushort", 2, False), ("sshort", 2, True)):
        w.v[0] = np.full(64, KEPT, np.uint32)
        run("global_load_%s v0, v1, s[4:5] offset:2" % op)
        for l in range(64):
            at = 3 * l + 3
            x = int.from_bytes(src[at:at + nb].tobytes(), "little")
            if signed and x >> (8 * nb - 1):
                x |= M32 & ~((1 << 8 * nb) - 1)
            assert int(w.v[0][l]) == (x if EXEC >> l & 1 else KEPT), (op, l)
    rd = mem.touched(base)[1]
    want = np.zeros(256, bool)
    for l in range(64):
        if EXEC >> l & 1:
            want[3 * l + 3:3 * l + 5] = True
    assert np.array_equal(rd, want)
    w.v[2] = np.arange(64, dtype=np.uint32) * np.uint32(0x01020304) + np.uint32(0xFFFEFDFC)
    run("global_store_byte v1, v2, s[6:7]")
    run("global_store_short v1, v2, s[6:7] offset:1")
    out, wr = mem.view(dstb, 256), mem.touched(dstb)[2]
    for l in range(64):
        at, x = 3 * l + 1, int(w.v[2][l])
        if EXEC >> l & 1:
            assert (int(out[at]), int(out[at + 1]) | int(out[at + 2]) << 8) == (x & 0xFF, x & 0xFFFF), l
            assert wr[at:at + 3].all()
        else:
            assert not wr[at:at + 3].any() and not out[at:at + 3].any(), l


def test_scratch_marks_record_uninitialised_reads():
    """Memory.declare_scratch: a read of a scratch byte no emulated store has written is recorded with its address and
    the instruction's line; reads of stored bytes, and of regions not declared, are not.  Off by default."""
    import wave_emu as E
    mem = E.Memory()
    a, b = mem.alloc(64, data=np.full(64, 0xA5, np.uint8)), mem.alloc(64)
    mem.read(a, 8)
    assert mem.scratch is None and mem.uninit == []
    mem.declare_scratch(a)
    mem.line = 17
    mem.write(a + 8, bytes(8))
    mem.read(a + 8, 8)
    mem.read(b, 8)
    assert mem.uninit == []
    mem.read(a + 12, 8)  # four stored bytes, four stale ones
    assert mem.uninit == [(a + 12, 8, 17)]
    mem.view(a, 64)[:] = 0  # the harness's own access initialises nothing
    mem.read(a, 1)
    assert mem.uninit[-1] == (a, 1, 17)
