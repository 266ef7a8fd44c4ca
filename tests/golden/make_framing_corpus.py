#!/usr/bin/env python3
"""Generate the corpus of damaged framing files and what the REFERENCE'S OWN readers make of each.

Runs only where the reference tree exists.  `make -C oracle framing` builds oracle/_ref/ref_framing_golden (the
reference's log::Reader, VlogReader and ReadBlock with its util/crc32c.cc, driven by tests/cpp/ref_framing_driver.cc);
its `corpus` mode applies a deterministic list of mutations to three base images and runs the reference reader on
every mutant.  This script runs it twice (the output must repeat byte for byte), checks the conditions below and
commits DATA only:

  framing_corpus_log.json    mutants of ref_manifest.log: the logical records log::Reader returned, every
                             Corruption(bytes, reason) it reported
  framing_corpus_vlog.json   mutants of ref_small.vlog: the records VlogReader returned and what it reported
  framing_corpus_sst.json    mutants of ref_table.sst: the blocks ReadBlock(verify_checksums) rejected, by index
  ref_small.vlog             the reference VlogWriter's file for payloads of 0, 1, 7, 8, 15, 16, 100, 4095, 4096,
                             65539 and 33 bytes (the repo's splitmix64 stream)

A mutation is applied in this order: cut the base to `cut` bytes (unless null), append `append` zero bytes, fill
[pos, pos + len) with a byte (`fills`: [pos, len, byte]), write single bytes (`writes`: [pos, byte]).  Checksums that a
mutant needs to be VALID over altered bytes were stamped by the driver with the reference's crc32c and are part of
`writes`, so a test never computes an expected value.  A returned record is [length, fnv64 of its bytes]; one that is
identical to record i of the intact image is stored as the integer i.

Conditions checked here (reference alone):
  * the regenerated base images are the committed ref_manifest.log / ref_table.sst byte for byte;
  * every class has at least one mutant whose reader output differs from the intact image's;
  * every log_chain_gap mutant makes the reference report "error in middle of record" or "missing start of
    fragmented record";
  * two runs give the same bytes; every written file is at most 512 KiB.
"""
import collections
import hashlib
import json
import os
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_framing_golden")
HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 512 * 1024


def run(d):
    return subprocess.run([DRIVER, "corpus", d], check=True, capture_output=True).stdout


def read(path):
    with open(path, "rb") as f:
        return f.read()


def compact(reader, intact):
    """A record equal to one of the intact image's records becomes that record's index."""
    index = {}
    for i, r in enumerate(intact["records"]):
        index.setdefault(tuple(r), i)
    return [index.get(tuple(r), r) for r in reader["records"]]


def classes_of(section, intact_output, output_of, entry_of):
    classes = collections.OrderedDict()
    differs = collections.Counter()
    for m in section["mutants"]:
        e = {k: m[k] for k in ("name", "cut", "append", "fills", "writes")}
        e.update(entry_of(m))
        classes.setdefault(m["class"], []).append(e)
        differs[m["class"]] += output_of(m) != intact_output
    for cls in classes:
        assert differs[cls] > 0, f"class {cls}: no mutant changes what the reference reader returns or reports"
    return classes


def build():
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        out = run(d1)
        assert out == run(d2), "the corpus differs between two runs"
        assert read(os.path.join(d1, "small_vlog.bin")) == read(os.path.join(d2, "small_vlog.bin"))
        assert read(os.path.join(d1, "manifest.log")) == read(os.path.join(HERE, "ref_manifest.log"))
        assert read(os.path.join(d1, "table.sst")) == read(os.path.join(HERE, "ref_table.sst"))
        vlog = read(os.path.join(d1, "small_vlog.bin"))
    j = json.loads(out)
    gen = "tests/golden/make_framing_corpus.py (oracle/_ref/ref_framing_golden corpus)"
    files = {"ref_small.vlog": vlog}

    lg = j["log"]
    for m in lg["mutants"]:
        if m["class"] == "log_chain_gap":
            why = " ".join(r for _, r in m["reader"]["drops"])
            assert "error in middle of record" in why or "missing start of fragmented record" in why, m["name"]
    log = {"generator": gen, "base": "ref_manifest.log",
           "base_sha256": hashlib.sha256(read(os.path.join(HERE, "ref_manifest.log"))).hexdigest(),
           "size": lg["size"], "reopen_at": lg["reopen_at"], "intact": lg["intact"],
           "classes": classes_of(lg, lg["intact"], lambda m: m["reader"],
                                 lambda m: {"records": compact(m["reader"], lg["intact"]),
                                            "drops": m["reader"]["drops"]})}
    vl = j["vlog"]
    assert vl["size"] == len(vlog)
    vj = {"generator": gen, "base": "ref_small.vlog", "base_sha256": hashlib.sha256(vlog).hexdigest(),
          "seed": vl["seed"], "lens": vl["lens"], "size": vl["size"], "intact": vl["intact"],
          "classes": classes_of(vl, vl["intact"], lambda m: m["reader"],
                                lambda m: {"records": compact(m["reader"], vl["intact"]),
                                           "drops": m["reader"]["drops"]})}
    ss = j["sst"]
    assert ss["intact_bad"] == []
    sj = {"generator": gen, "base": "ref_table.sst",
          "base_sha256": hashlib.sha256(read(os.path.join(HERE, "ref_table.sst"))).hexdigest(),
          "size": ss["size"], "blocks": ss["blocks"], "intact_bad": ss["intact_bad"],
          "classes": classes_of(ss, ss["intact_bad"], lambda m: m["bad"], lambda m: {"bad": m["bad"]})}
    for name, doc in (("framing_corpus_log.json", log), ("framing_corpus_vlog.json", vj),
                      ("framing_corpus_sst.json", sj)):
        files[name] = (json.dumps(doc, separators=(",", ":")) + "\n").encode()
    for name, data in files.items():
        assert len(data) <= LIMIT, (name, len(data))
    return files, {name[len("framing_corpus_"):-5]: {c: len(v) for c, v in doc["classes"].items()}
                   for name, doc in (("framing_corpus_log.json", log), ("framing_corpus_vlog.json", vj),
                                     ("framing_corpus_sst.json", sj))}


def main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "framing"])
    files, counts = build()
    again, _ = build()
    assert files == again, "the fixtures differ between two generations"
    for name, data in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        print(f"wrote {name}: {len(data)} bytes")
    for fmt, c in counts.items():
        print(fmt, "mutants per class:", ", ".join(f"{k} {v}" for k, v in c.items()))


if __name__ == "__main__":
    main()
