"""The reference-recorded corpus of damaged framing files (tests/golden/framing_corpus_*.json, written by
tests/golden/make_framing_corpus.py from the reference's own readers) -- TEST INFRASTRUCTURE shared by
test_framing_reference_cpu.py and test_gpu_framing_corpus.py.  Nothing here computes an expected value: the mutants'
bytes come from the committed base image plus the recorded mutation, the expectations from the recorded reader output;
the only checksums computed are the library's own host leg (kvsep_crc32c_extend_host), i.e. the code under test."""
import hashlib
import json
import os

import numpy as np

import kvsep
from framing_builders import assemble, fnv64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISMATCH = "Corruption: checksum mismatch"
BAD_LENGTH = "Corruption: bad record length"
_CACHE = {}


def load(fmt):
    """(corpus document, base image) of "log", "vlog" or "sst"; a missing or altered file raises (a failure)."""
    if fmt not in _CACHE:
        with open(os.path.join(GOLDEN, f"framing_corpus_{fmt}.json")) as f:
            doc = json.load(f)
        with open(os.path.join(GOLDEN, doc["base"]), "rb") as f:
            base = f.read()
        assert len(base) == doc["size"] and hashlib.sha256(base).hexdigest() == doc["base_sha256"], doc["base"]
        _CACHE[fmt] = (doc, base)
    return _CACHE[fmt]


def classes(fmt):
    """Class names for parametrize; a missing corpus yields one name whose test then fails in load()."""
    try:
        return list(load(fmt)[0]["classes"])
    except Exception:
        return [f"{fmt}_corpus_missing"]


def mutate(base: bytes, m) -> bytes:
    b = bytearray(base)
    if m["cut"] is not None:
        del b[m["cut"]:]
    b += bytes(m["append"])
    for pos, n, byte in m["fills"]:
        b[pos:pos + n] = bytes([byte]) * n
    for pos, byte in m["writes"]:
        b[pos] = byte
    return bytes(b)


def describe(cls, m):
    w = m["writes"] if len(m["writes"]) <= 8 else m["writes"][:8] + ["..."]
    return f"class {cls}, mutant '{m['name']}' (cut={m['cut']} append={m['append']} fills={m['fills']} writes={w})"


def want_records(m, intact):
    return [intact["records"][r] if isinstance(r, int) else r for r in m["records"]]


def reported(m, reason):
    return sum(n for n, why in m["drops"] if why == reason)


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"record {i}: got {g}, reference {w}"
    if len(got) != len(want):
        i = min(len(got), len(want))
        return f"record {i}: got {got[i] if i < len(got) else 'none'}, reference {want[i] if i < len(want) else 'none'}"
    return None


def host_crcs(img: bytes, off, ln):
    """The library's host leg over [off, off + len) of the image, one kvsep_crc32c_extend_host call per record."""
    a = np.frombuffer(img, dtype=np.uint8) if len(img) else np.zeros(1, np.uint8)
    f = kvsep.lib().kvsep_crc32c_extend_host
    return np.array([f(0, a.ctypes.data + int(o), int(n)) for o, n in zip(off, ln)], dtype=np.uint32)


def log_host_ok(img, off, ln, stored):
    crc = host_crcs(img, off, ln)
    return np.array([1 if int(c) == kvsep.unmask(int(s)) else 0 for c, s in zip(crc, stored)], dtype=np.uint8)


def check_log(cls, m, img, intact, walk, ok):
    """accept + assembly over the walk and the verdicts ok[] against what log::Reader returned and reported."""
    off, ln, _, ty = walk
    accept, gap, dropped, bad_len = kvsep.log_accept_gaps(img, ok)
    accept0, dropped0 = kvsep.log_accept(off, ok, len(img))
    what = describe(cls, m)
    if not any(o and t in (5, 6) for o, t in zip(ok, ty)):  # kvsep_log_accept sees no types: the reader's kEof /
        assert np.array_equal(accept, accept0) and dropped == dropped0, what  # kBadRecord codes are beyond it
    diff = first_difference(assemble(img, off, ln, ty, accept, gap), want_records(m, intact))
    assert diff is None, f"{what}: {diff}"
    assert dropped == reported(m, MISMATCH), f"{what}: checksum-mismatch bytes"
    assert bad_len == reported(m, BAD_LENGTH), f"{what}: bad-record-length bytes"


def vlog_expect(m, intact):
    """(ngood, good_bytes, drop_bytes, a mismatch was reported) as VlogReader saw them: the records it returned (header
    + payload each) lie back to back from offset 0."""
    recs = want_records(m, intact)
    hits = [n for n, why in m["drops"] if why == MISMATCH]
    assert len(hits) <= 1 and len(hits) == len(m["drops"])  # the only thing VlogReader reports, and it stops there
    return len(recs), sum(r[0] for r in recs), sum(hits), bool(hits)


def vlog_records(img, off, ln, ngood):
    return [[int(ln[i]) + 8, fnv64(img[int(off[i]) - 8:int(off[i] + ln[i])])] for i in range(ngood)]


def sst_host_bad(img, blocks):
    """Blocks whose mask(Value(block || type)) differs from the stored trailer word, by the library's host leg."""
    off = [b[0] for b in blocks]
    crc = host_crcs(img, off, [b[1] + 1 for b in blocks])
    return [i for i, (c, (o, n)) in enumerate(zip(crc, blocks))
            if kvsep.mask(int(c)) != int.from_bytes(img[o + n + 1:o + n + 5], "little")]
