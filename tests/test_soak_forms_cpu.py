"""The forms soak (kv-separate_amd/tools/soak_forms.py) without a device: what keeps a wrong model, a generator that
misses its edges or a blind comparator from turning up later as a false pass or a false failure on the GPU.

  models      every committed case of a family that has a host form goes through that form (kvsep.combine,
              vlog_frame_offsets, log_frame_layout, sst_index_build, sst_footer_build, log_walk, log_accept_gaps, log_chains, sst_footer, sst_index_walk,
              sst_index_keys) and is compared with expect(case)
              by the soak's own compare(): a new differential check of framing.cpp as well;
  generators  over the committed seeds and counts every family reaches its edge classes; every generated case has a model
              (none is skipped or filtered), respects the size limits and depends on (family, seed, index) alone;
  comparator  one output word off by one, one destination byte flipped, one canary byte written, one byte past the
              written range inside dst: compare() raises and names the array and the index."""
import os
import sys

import numpy as np
import pytest

import kvsep

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kv-separate_amd", "tools"))
import soak_forms as S  # noqa: E402
from soak_forms_counts import CASES, SEEDS  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    """Every committed case with its expectation, computed once and left unchanged."""
    out = {}
    for f in S.FAMILIES:
        out[f] = [(c, S.expect(c)) for seed in SEEDS for c in (S.make_case(f, seed, k) for k in range(CASES[f]))]
    return out


def singles(cases):
    for f in S.SINGLE:
        yield from cases[f]
    for f in ("sequence", "captured"):
        for c, wants in cases[f]:
            yield from zip(c.members, wants)


# ------------------------------------------------------------------------------------------------ the host forms
def host_combine(c):
    """The fold of kvsep_crc32c_combine over each run, with the segments' CRCs the model gives (or the case holds)."""
    ln, init = c.inp["seg_len"], c.inp.get("init")
    crc = c.inp["seg_crc"] if c.form == "concat" else S.oracle().batch(S._base(c), c.inp["seg_off"], ln)
    out = np.zeros(c.par["count"], np.uint32)
    for i, (lo, hi) in enumerate(run_bounds(c)):
        acc = 0 if init is None else int(init[i])
        for j in range(lo, hi):
            acc = kvsep.combine(acc, int(crc[j]), int(ln[j]))
        out[i] = acc
    return dict(out=out)


def run_bounds(c):
    """The header's reading of first[], restated here and not taken from the model: every value clamped to nseg, a run
    that ends before it starts empty.  (kvsep.combine itself is only ever a fold: the device's reading of a wild
    first[] is checked on the GPU alone.)"""
    first, nseg = [int(x) for x in c.inp["first"]], c.par["nseg"]
    return [(min(a, nseg), max(min(a, nseg), min(b, nseg))) for a, b in zip(first, first[1:])]


def host_vlog_frame_auto(c):
    lens = [int(c.inp["seg_len"][lo:hi].sum()) for lo, hi in run_bounds(c)]
    rec_off, end = kvsep.vlog_frame_offsets(lens, c.par["start"])
    return dict(rec_off=rec_off, end=np.array([end], np.uint64))


def host_log_frame(c):
    rec_at, first, nfrag, written = kvsep.log_frame_layout(c.inp["len"], c.inp.get("keep"), c.par["dest_length"])
    return dict(rec_at=rec_at, frag_first=first, nfrag=np.array([nfrag], np.uint64),
                written=np.array([written], np.uint64))


def host_sst_index_build(c):
    dst = np.full(c.par["dst_bytes"], S.CANARY, np.uint8)
    _, out_len, st = kvsep.sst_index_build(S._base(c), c.inp["key_off"], c.inp["key_len"], c.inp["blk_off"],
                                           c.inp["blk_len"], c.inp.get("keep"), dst=dst, at=int(c.inp["at"][0]))
    return dict(dst=dst, out_len=np.array([out_len], np.uint64), status=np.array([st], np.uint32))


def host_sst_table_finish(c):
    """The table from the host builder's parts: the empty block, the index block, kvsep_sst_footer_build."""
    at = int(c.inp["at"][0])
    idx, out_len, st = kvsep.sst_index_build(S._base(c), c.inp["key_off"], c.inp["key_len"], c.inp["blk_off"],
                                             c.inp["blk_len"], c.inp.get("keep"))
    assert st == kvsep.SSTW_OK
    z = np.zeros(0, np.uint64)
    meta, meta_len, st = kvsep.sst_index_build(b"\0", z, z, z, z)
    assert (st, meta_len) == (kvsep.SSTW_OK, 8)
    table = meta + idx + kvsep.sst_footer_build((at, meta_len), (at + 13, out_len))
    dst = np.full(c.par["dst_bytes"], S.CANARY, np.uint8)
    fits = at + len(table) <= dst.size
    if fits:
        dst[at:at + len(table)] = np.frombuffer(table, np.uint8)
    return dict(dst=dst, out_len=np.array([out_len], np.uint64),
                table_bytes=np.array([at + len(table) if fits else 0], np.uint64))


def _padded(a, cap, dtype, fill=0):
    out = np.full(cap, fill, dtype)
    out[:min(len(a), cap)] = np.asarray(a)[:cap]
    return out


def host_log(c, want):
    """kvsep_log_walk, kvsep_log_accept_gaps and kvsep_log_chains, chained as the device forms chain them."""
    cap, got = c.par["cap"], {}
    img = S._base(c)[:c.par["n"]].tobytes()
    if c.form != "log_chains":
        off, ln, st, ty = kvsep.log_walk(img)
        cnt = min(off.size, cap)
        got.update(off=_padded(off, cap, np.uint64), len=_padded(ln, cap, np.uint64), stored=_padded(st, cap, np.uint32),
                   type=_padded(ty, cap, np.uint8), nrec=np.array([off.size], np.uint64))
        ok = c.inp["w_ok"] if c.form == "log_accept_gaps" else want["ok"] if "ok" in want else None
        if ok is not None:  # the checksum verdicts are the oracle's (or the caller's): the rule is what is compared
            acc, gap, dropped, bad = kvsep.log_accept_gaps(img, ok[:cnt])
            got.update(accept=_padded(acc, cap, np.uint8), gap=_padded(gap, cap, np.uint8),
                       dropped=np.array([dropped], np.uint64), bad_length=np.array([bad], np.uint64))
        ty, acc, gap = got["type"], got.get("accept"), got.get("gap")
    else:
        cnt = min(int(c.inp["w_nrec"][0]), cap)
        ty, acc, gap = c.inp["w_type"], c.inp["w_accept"], c.inp.get("w_gap")
    if "first" in c.out:
        first, whole, nchain, nwhole = kvsep.log_chains(ty[:cnt], acc[:cnt], None if gap is None else gap[:cnt])
        got.update(first=_padded(first, cap + 1, np.uint64, cnt), whole=_padded(whole, cap, np.uint8),
                   nchain=np.array([nchain], np.uint64), nwhole=np.array([nwhole], np.uint64))
    return {k: v for k, v in got.items() if k in c.out}


def host_sst(c, want):
    """kvsep_sst_footer for the table form; kvsep_sst_index_walk / kvsep_sst_index_keys over the block the handle names."""
    cap, img = c.par["cap"], S._base(c)[:c.par["n"]].tobytes()
    if c.form == "sst_table_verify":
        handles, st = kvsep.sst_footer(img)
        assert (st == kvsep.SST_BAD_FOOTER) == (int(want["status"][0]) == kvsep.SST_BAD_FOOTER), c.line()
        return dict(handles=np.array(handles, np.uint64))
    ioff, ilen = (int(x) for x in c.inp["handle"])
    if ioff + ilen + 5 > len(img):  # the footer's rule, not the walk's: no host walk to ask
        return {}
    block = img[ioff:ioff + ilen]
    if c.form == "sst_index":
        off, ln, nb, st = kvsep.sst_index_walk(block, cap=cap)
        got = dict(off=off, len=ln)
    else:
        off, ln, koff, klen, nb, st = kvsep.sst_index_keys(block, cap=cap)
        koff = koff.copy()
        koff[:min(nb, cap)] += np.uint64(ioff)  # the host form counts from the block, the device form from the image
        got = dict(off=off, len=ln, key_off=koff, key_len=klen)
    got.update(nblocks=np.array([nb], np.uint64), status=np.array([st], np.uint32))
    return got


HOST = {"sst_index": host_sst, "sst_index_keys": host_sst, "sst_table_verify": host_sst, "log_walk": host_log, "log_read": host_log, "log_accept_gaps": host_log, "log_chains": host_log,
        "log_records": host_log, "concat": host_combine, "gather": host_combine, "vlog_frame_auto": host_vlog_frame_auto,
        "log_frame": host_log_frame, "log_frame_records": host_log_frame, "sst_index_build": host_sst_index_build,
        "sst_table_finish": host_sst_table_finish}


def test_models_agree_with_the_host_forms(cases):
    seen = set()
    for c, want in singles(cases):
        if c.form in HOST:
            got = HOST[c.form](c, want) if HOST[c.form] in (host_log, host_sst) else HOST[c.form](c)
            S.compare(c, S.as_got(c, got), want, only=set(got))
            seen.add(c.form)
    assert seen == set(HOST)


# ------------------------------------------------------------------------------------------------ the generators
COUNTS = {"count0", "count1", "count_big"}
REACH = {
    "lists": COUNTS | {"skew", "bad_none", "bad_some", "bad_all", "cap_below", "cap_at", "cap_above", "ok", "no_ok"},
    "combine": COUNTS | {"skew", "run31", "run32", "run33", "run_empty", "seg_empty", "first_wild", "init", "no_init"},
    "frame": COUNTS | {"skew", "dst_skew", "long_segment", "refusal:dst_short"},
    "layout": COUNTS | {"skew", "dst_skew", "refusal:dst_short", "rule_all", "rule_keep", "rule_before", "first",
                        "huge_huge", "huge_skip", "huge_two_halves", "huge_start", "saturated"},
    "logread": COUNTS | {"skew", "dst_skew", "refusal:dst_short", "cap_below", "cap_at", "cap_above", "two_damages",
                         "block_tail", "chains_random", "type_with_good_checksum"} | {"damage_" + d for d in S.DAMAGES},
    "logwrite": COUNTS | {"skew", "dst_skew", "refusal:dst_short", "refusal:frag_cut", "fragcap_below", "fragcap_at",
                          "fragcap_above", "keep_skip", "block_tail", "many_fragments"},
    "sstread": COUNTS | {"skew", "interval1", "interval2", "interval16", "cap_below", "cap_at", "cap_above",
                         "damage_data", "damage_index", "index_compressed", "refusal:bad_footer",
                         "refusal:shared_key"},
    "sstwrite": COUNTS | {"skew", "dst_skew", "refusal:no_room", "staged_and_unstaged", "several_unstaged", "keep",
                          "blk_skip", "refusal:source", "rewrite_cap_below", "rewrite_cap_at", "rewrite_cap_above"},
    "sequence": {"grown_by_two_forms"},
    "captured": {"grown_by_two_forms", "refusal:over_reservation"},
}


def test_generators_reach_the_edges(cases):
    for f in S.FAMILIES:
        assert len(cases[f]) == len(SEEDS) * CASES[f]  # none skipped, none filtered
        reached = set()
        for c, want in cases[f]:
            reached |= c.edges
            if f == "layout" and c.form == "offsets" and int(want["end"][0]) == S.U64:
                reached.add("saturated")  # from the model's own result, not from what the generator meant
        assert REACH[f] <= reached, f"{f}: not reached: {sorted(REACH[f] - reached)}"
    forms = {c.form for c, _ in singles(cases)}
    assert forms == set(S.MODELS)
    members = [len(c.members) for f in ("sequence", "captured") for c, _ in cases[f]]
    assert min(members) >= 6 and max(members) <= 10


def test_cases_respect_the_limits_and_depend_on_their_index_alone(cases):
    for c, _ in singles(cases):
        assert c.elements <= S.MAX_ELEMENTS and c.nbytes <= S.MAX_PAYLOAD, c.line()
        assert all(a.size <= S.MAX_ELEMENTS + 1 for n, a in c.inp.items() if n != "src"), c.line()
    for f in S.FAMILIES:
        c, _ = cases[f][CASES[f] // 2]
        again = S.make_case(f, c.seed, c.index)  # built alone, after and before nothing
        assert again.line() == c.line()
        for a, b in zip(again.members or [again], c.members or [c]):
            assert a.par == b.par and sorted(a.inp) == sorted(b.inp)
            assert all(np.array_equal(a.inp[k], b.inp[k]) for k in a.inp)


# ------------------------------------------------------------------------------------------------ the comparator
def planted(c, want):
    """(kind, array, index, the perturbed device result) for every kind this case has room for."""
    for name in sorted(want):
        n = c.out[name][1]
        lo = S.guard_lo(c, name)
        if name != "dst" and n:
            got = S.as_got(c, want)
            got[name][lo + n - 1] ^= 1  # off by one
            yield "word", name, n - 1, got
        if name != "dst":
            got = S.as_got(c, want)
            got[name][lo + n] ^= 1
            yield "guard", name, n, got
    if "dst" in want:
        n, lo = c.out["dst"][1], S.guard_lo(c, "dst")
        written = np.flatnonzero(want["dst"] != S.CANARY)
        if written.size:
            got = S.as_got(c, want)
            got["dst"][lo + written[0]] ^= 0x10
            yield "byte", "dst", int(written[0]), got
            if written[-1] + 1 < n:  # one byte beyond the written range, still inside dst
                got = S.as_got(c, want)
                got["dst"][lo + written[-1] + 1] = 0
                yield "beyond", "dst", int(written[-1]) + 1, got
        for at in (-1, n):  # the canary bytes on either side
            got = S.as_got(c, want)
            got["dst"][lo + at] = 0
            yield "canary", "dst", at, got
    name = sorted(c.inp)[0]
    if c.inp[name].size:
        got = S.as_got(c, want)
        got["in:" + name].reshape(-1)[0] ^= 1
        yield "input", "in:" + name, 0, got


def test_a_refused_call_must_leave_everything_as_it_was(cases):
    c = next(c for c, _ in cases["captured"] if c.refused)
    m, want = c.refused, S.expect_refused(c.refused)
    S.compare(m, S.as_got(m, want), want)
    got = S.as_got(m, S.expect(m))  # the call went through after all
    with pytest.raises(S.Mismatch):
        S.compare(m, got, want)


def test_the_comparator_notices(cases):
    for f in S.SINGLE:
        kinds = set()
        for c, want in cases[f][:12]:
            S.compare(c, S.as_got(c, want), want)
            for kind, name, index, got in planted(c, want):
                with pytest.raises(S.Mismatch) as e:
                    S.compare(c, got, want)
                assert (e.value.array, e.value.index) == (name, index), (c.line(), kind)
                assert c.id in str(e.value) and f"{name}[{index}]" in str(e.value)
                kinds.add(kind)
        assert {"word", "guard", "input"} <= kinds, f
        if f in ("frame", "layout", "logread", "logwrite", "sstwrite"):
            assert {"byte", "beyond", "canary"} <= kinds, f
