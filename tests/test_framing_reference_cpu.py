"""The framing READERS against the reference's own readers on a corpus of damaged files (no GPU).

tests/golden/framing_corpus_{log,vlog,sst}.json hold, per mutation of a reference-written base image, what the
reference's log::Reader, VlogReader and ReadBlock returned and reported (tests/golden/make_framing_corpus.py).  Every
mutant is rebuilt from the committed base and run through the library's host walkers and host checksum leg:

  log    kvsep_log_walk, ok[i] = (kvsep_crc32c_extend_host over [off, len) == unmask(stored)), kvsep_log_accept_gaps
         and the documented assembly loop (framing_builders.assemble) give log::Reader's logical records, its
         "checksum mismatch" bytes and its "bad record length" bytes; kvsep_log_accept agrees on accept[] and the bytes.
  vlog   kvsep_vlog_walk plus the host leg give VlogReader's record count, its records and its mismatch bytes.
  SST    mask(Value(block || type)) == stored flags exactly the blocks ReadBlock rejected.

One test per mutation class; a failure names the class, the mutation and the first differing record.
"""
import pytest

import kvsep
import framing_corpus as FC


@pytest.mark.parametrize("cls", FC.classes("log"))
def test_log_readers_match_reference(cls):
    doc, base = FC.load("log")
    for m in doc["classes"][cls]:
        img = FC.mutate(base, m)
        walk = kvsep.log_walk(img)
        off, ln, stored, _ = walk
        FC.check_log(cls, m, img, doc["intact"], walk, FC.log_host_ok(img, off, ln, stored))


def test_log_intact_image_matches_reference():
    doc, base = FC.load("log")
    m = {"name": "intact", "cut": None, "append": 0, "fills": [], "writes": [],
         "records": list(range(len(doc["intact"]["records"]))), "drops": doc["intact"]["drops"]}
    walk = kvsep.log_walk(base)
    FC.check_log("intact", m, base, doc["intact"], walk, FC.log_host_ok(base, walk[0], walk[1], walk[2]))


@pytest.mark.parametrize("cls", FC.classes("vlog"))
def test_vlog_readers_match_reference(cls):
    doc, base = FC.load("vlog")
    for m in doc["classes"][cls]:
        img = FC.mutate(base, m)
        what = FC.describe(cls, m)
        off, ln, stored, _ = kvsep.vlog_walk(img)
        crc = FC.host_crcs(img, off, ln)
        good = 0
        while good < off.size and kvsep.mask(int(crc[good])) == int(stored[good]):
            good += 1
        ngood, _, drop, hit = FC.vlog_expect(m, doc["intact"])
        assert good == ngood, f"{what}: {good} good records, reference {ngood}"
        diff = FC.first_difference(FC.vlog_records(img, off, ln, good), FC.want_records(m, doc["intact"]))
        assert diff is None, f"{what}: {diff}"
        assert (good < off.size) == hit, f"{what}: a checksum mismatch was reported"
        assert (int(ln[good]) if good < off.size else 0) == drop, f"{what}: checksum-mismatch bytes"


@pytest.mark.parametrize("cls", FC.classes("sst"))
def test_sst_read_check_matches_reference(cls):
    doc, base = FC.load("sst")
    for m in doc["classes"][cls]:
        img = FC.mutate(base, m)
        assert FC.sst_host_bad(img, doc["blocks"]) == m["bad"], FC.describe(cls, m)


def test_corpus_bites():
    """Every class holds a mutant on which the reference's output differs from the intact image's, and the chain-gap
    class only mutants on which log::Reader reported a broken fragment chain (the generator's conditions, rechecked
    on the committed data)."""
    for fmt in ("log", "vlog"):
        doc, _ = FC.load(fmt)
        n = len(doc["intact"]["records"])
        for cls, ms in doc["classes"].items():
            assert any(m["records"] != list(range(n)) or m["drops"] for m in ms), cls
    doc, _ = FC.load("sst")
    for cls, ms in doc["classes"].items():
        assert any(m["bad"] for m in ms), cls
    for m in FC.load("log")[0]["classes"]["log_chain_gap"]:
        why = " ".join(r for _, r in m["drops"])
        assert "error in middle of record" in why or "missing start of fragmented record" in why, m["name"]
