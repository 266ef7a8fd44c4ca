// ref_framing_driver.cc -- TEST INFRASTRUCTURE ONLY (never shipped, never measured).
//
// Drives the reference's OWN framing code, compiled unchanged from /root/reference by oracle/Makefile:
//   db/value_log_writer.cc:33-76 / db/value_log_reader.cc:64-138   vlog records
//   db/log_writer.cc:23-115 / db/log_reader.cc:58-272              MANIFEST (log) records, 32 KiB blocks
//   table/table_builder.cc:83-232 / table/format.cc:73-155         SST blocks and their 5-byte trailers
// It is linked twice (oracle/Makefile `framing`):
//   oracle/_ref/ref_framing_golden   with the reference's util/crc32c.cc: writes the golden files and the readers'
//                                    verdicts on corrupted copies (tests/golden/make_framing_golden.py commits them);
//   oracle/_ref/ref_framing_kvsep    with util/crc32c.cc replaced by libkvsep_crc32c.so (its exported
//                                    leveldb::crc32c::Extend): the same call sites on this engine.  With "gpu"
//                                    every Extend -- down to InitTypeCrc's 1-byte ones -- goes through the GPU
//                                    (offload threshold 0) and the run checks that none fell back to the host.
// Both builds print the same JSON for the same inputs iff the engine is bit-exact at every call site.
//
// usage: <binary> <out_dir> [gpu]
//        <binary> corpus [out_dir]     the corpus of damaged files and the reference readers' output on each
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "db/log_reader.h"
#include "db/log_writer.h"
#include "db/value_log_reader.h"
#include "db/value_log_writer.h"
#include "leveldb/env.h"
#include "leveldb/options.h"
#include "leveldb/table_builder.h"
#include "table/format.h"
#include "util/crc32c.h"

#ifdef KVSEP_CALLSITE
#include "kvsep_crc32c.h"
#endif

using leveldb::Slice;
using leveldb::Status;

namespace {

// The repo's synthetic byte stream (kvsep/workloads.py): byte i = byte (i & 7) of splitmix64 word (i >> 3).
uint64_t splitmix_word(uint64_t seed, uint64_t j) {
  uint64_t z = seed + (j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
std::string stream_bytes(uint64_t seed, uint64_t off, uint64_t n) {
  std::string s(n, '\0');
  for (uint64_t i = 0; i < n; ++i) s[i] = char(splitmix_word(seed, (off + i) >> 3) >> (8 * ((off + i) & 7)));
  return s;
}

uint64_t fnv64(const char* p, size_t n) {  // record identity in the JSON (independent of the CRC under test)
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ uint8_t(p[i])) * 0x100000001b3ull;
  return h;
}

class StringSink : public leveldb::WritableFile {
 public:
  std::string contents;
  std::vector<std::pair<uint64_t, uint64_t>> appends;  // (offset, size) of every Append
  Status Append(const Slice& d) override {
    appends.emplace_back(contents.size(), d.size());
    contents.append(d.data(), d.size());
    return Status::OK();
  }
  Status Close() override { return Status::OK(); }
  Status Flush() override { return Status::OK(); }
  Status Sync() override { return Status::OK(); }
  size_t GetSize() override { return contents.size(); }
};

class StringSource : public leveldb::SequentialFile {
 public:
  explicit StringSource(const std::string& s) : data_(s) {}
  Status Read(size_t n, Slice* result, char* scratch) override {
    const size_t k = std::min<size_t>(n, data_.size() - pos_);
    std::memcpy(scratch, data_.data() + pos_, k);
    pos_ += k;
    *result = Slice(scratch, k);
    return Status::OK();
  }
  Status Skip(uint64_t n) override {
    pos_ = std::min<size_t>(data_.size(), pos_ + n);
    return Status::OK();
  }

 private:
  const std::string& data_;
  size_t pos_ = 0;
};

class StringRandom : public leveldb::RandomAccessFile {
 public:
  explicit StringRandom(const std::string& s) : data_(s) {}
  Status Read(uint64_t offset, size_t n, Slice* result, char* scratch) const override {
    if (offset > data_.size()) return Status::IOError("offset past end");
    const size_t k = std::min<size_t>(n, data_.size() - offset);
    std::memcpy(scratch, data_.data() + offset, k);
    *result = Slice(scratch, k);
    return Status::OK();
  }

 private:
  const std::string& data_;
};

struct Drops {
  std::vector<std::pair<size_t, std::string>> v;
  std::string json() const {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) {
      char b[64];
      std::snprintf(b, sizeof b, "%s[%zu,", i ? "," : "", v[i].first);
      s += b;
      s += "\"" + v[i].second + "\"]";
    }
    return s + "]";
  }
};

struct VlogReporter : leveldb::log::VlogReader::Reporter {
  Drops d;
  void Corruption(size_t bytes, const Status& st) override { d.v.emplace_back(bytes, st.ToString()); }
};

struct LogReporter : leveldb::log::Reader::Reporter {
  Drops d;
  void Corruption(size_t bytes, const Status& st) override { d.v.emplace_back(bytes, st.ToString()); }
};

bool write_file(const std::string& path, const std::string& s) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(s.data(), 1, s.size(), f) == s.size();
  return std::fclose(f) == 0 && ok;
}

std::string hex(const char* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[uint8_t(p[i]) >> 4];
    s += d[uint8_t(p[i]) & 15];
  }
  return s;
}

// ------------------------------------------------------------------ vlog
constexpr uint64_t kVlogSeed = 0x766c6f67;
const uint64_t kVlogLens[] = {0, 1, 7, 8, 15, 16, 100, 4095, 4096, 65539, 1048609, 1048609, 1048609, 300001, 33};
constexpr size_t kVlogN = sizeof(kVlogLens) / sizeof(kVlogLens[0]);

// Records VlogReader returns (header + payload each, db/value_log_reader.cc:101,126) and what it reported.
std::string vlog_read(const std::string& img) {
  StringSource src(img);
  VlogReporter rep;
  leveldb::log::VlogReader r(&src, &rep, true, 0);
  Slice rec;
  std::string scratch;
  std::string out = "[";
  int k = 0;
  while (r.ReadRecord(&rec, &scratch)) {
    char b[64];
    std::snprintf(b, sizeof b, "%s[%zu,\"%016llx\"]", k++ ? "," : "", rec.size(),
                  (unsigned long long)fnv64(rec.data(), rec.size()));
    out += b;
  }
  return "{\"records\":" + out + "],\"drops\":" + rep.d.json() + "}";
}

// The reference VlogWriter over payloads of these lengths cut from the splitmix stream; *offs (nullable) = the
// offsets AddRecord returned, as a JSON list.
std::string build_vlog(const uint64_t* lens, size_t n, std::string* offs) {
  StringSink sink;
  leveldb::log::VlogWriter w(&sink);
  uint64_t pos = 0;
  if (offs) *offs = "[";
  for (size_t i = 0; i < n; ++i) {
    const std::string p = stream_bytes(kVlogSeed, pos, lens[i]);
    pos += lens[i];
    uint64_t off = 0;
    if (!w.AddRecord(Slice(p), off).ok()) std::abort();
    if (offs) *offs += (i ? "," : "") + std::to_string(off);
  }
  if (offs) *offs += "]";
  return sink.contents;
}

std::string vlog_section(const std::string& dir) {
  std::string offs;
  const std::string img = build_vlog(kVlogLens, kVlogN, &offs);
  if (!dir.empty() && !write_file(dir + "/vlog.bin", img)) std::abort();
  std::string headers = "[";
  for (size_t i = 0, p = 0; i < kVlogN; p += 8 + kVlogLens[i], ++i) headers += (i ? ",\"" : "\"") + hex(&img[p], 8) + "\"";
  headers += "]";
  // corrupted copies: a payload byte of record 11, the stored CRC of record 3, the low length byte of record 9,
  // and a torn tail (the last record cut short)
  auto rec_at = [&](size_t k) {
    uint64_t p = 0;
    for (size_t i = 0; i < k; ++i) p += 8 + kVlogLens[i];
    return p;
  };
  struct Case {
    const char* name;
    uint64_t flip;  // byte XOR 0x80 at this offset, or
    uint64_t cut;   // truncate to this size (0 = no)
  };
  const Case cases[] = {{"payload_r11", rec_at(11) + 8 + 524288, 0},
                        {"crc_r3", rec_at(3) + 1, 0},
                        {"len_r9", rec_at(9) + 4, 0},
                        {"torn_tail", 0, img.size() - 5}};
  std::string cs = "[";
  for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c) {
    std::string bad = img;
    if (cases[c].cut) bad.resize(cases[c].cut);
    else bad[cases[c].flip] ^= char(0x80);
    char b[128];
    std::snprintf(b, sizeof b, "%s{\"name\":\"%s\",\"flip\":%llu,\"cut\":%llu,\"reader\":", c ? "," : "", cases[c].name,
                  (unsigned long long)cases[c].flip, (unsigned long long)cases[c].cut);
    cs += b + vlog_read(bad) + "}";
  }
  cs += "]";
  std::string lens = "[";
  for (size_t i = 0; i < kVlogN; ++i) lens += (i ? "," : "") + std::to_string(kVlogLens[i]);
  lens += "]";
  return "{\"seed\":" + std::to_string(kVlogSeed) + ",\"lens\":" + lens + ",\"offsets\":" + offs +
         ",\"size\":" + std::to_string(img.size()) + ",\"headers\":" + headers + ",\"intact\":" + vlog_read(img) +
         ",\"cases\":" + cs + "}";
}

// ------------------------------------------------------------------ log / MANIFEST
constexpr uint64_t kLogSeed = 0x6d616e69;
constexpr uint64_t kBlock = 32768, kHeader = 7;

std::string log_read(const std::string& img) {
  StringSource src(img);
  LogReporter rep;
  leveldb::log::Reader r(&src, &rep, true, 0);
  Slice rec;
  std::string scratch, out = "[";
  int k = 0;
  while (r.ReadRecord(&rec, &scratch)) {
    char b[64];
    std::snprintf(b, sizeof b, "%s[%zu,\"%016llx\"]", k++ ? "," : "", rec.size(),
                  (unsigned long long)fnv64(rec.data(), rec.size()));
    out += b;
  }
  return "{\"records\":" + out + "],\"drops\":" + rep.d.json() + "}";
}

struct LogImage {
  std::string img;
  std::vector<uint64_t> lens;  // logical record lengths
  std::vector<int> writer_of;  // 0 = the first writer, 1 = the one reopened at reopen_at
  uint64_t reopen_at = 0;
};

LogImage build_log() {
  // Lengths are chosen from the block offset so that every fragment type and every trailer case appears:
  // block trailers of 3 and 6 zero bytes, a record starting with exactly 7 bytes left in its block (a FIRST
  // fragment of 0 bytes, db/log_writer.cc:47-58), FIRST/MIDDLE/LAST chains, an empty record; then the log is
  // reopened with dest_length (the MANIFEST-reuse constructor, db/log_writer.cc:25-28) and appended to.
  LogImage L;
  StringSink sink;
  std::vector<uint64_t>& lens = L.lens;
  std::vector<int>& writer_of = L.writer_of;
  uint64_t pos = 0;
  auto boff = [&] { return sink.contents.size() % kBlock; };
  auto add = [&](leveldb::log::Writer& w, uint64_t n, int wi) {
    const std::string p = stream_bytes(kLogSeed, pos, n);
    pos += n;
    if (!w.AddRecord(Slice(p)).ok()) std::abort();
    lens.push_back(n);
    writer_of.push_back(wi);
  };
  auto leave = [&](uint64_t k) { return kBlock - boff() - kHeader - k; };  // record length leaving k bytes
  {
    leveldb::log::Writer w(&sink);
    add(w, 100, 0);
    add(w, leave(3), 0);   // 3-byte trailer
    add(w, 50000, 0);      // FIRST + LAST
    add(w, 0, 0);          // empty FULL record
    add(w, leave(6), 0);   // 6-byte trailer
    add(w, 100000, 0);     // FIRST + MIDDLE + MIDDLE + LAST
    add(w, leave(7), 0);   // exactly a header's room left ...
    add(w, 5000, 0);       // ... so this starts with a 0-byte FIRST fragment
  }
  L.reopen_at = sink.contents.size();
  {
    leveldb::log::Writer w(&sink, L.reopen_at);
    add(w, 1, 1);
    add(w, 70000, 1);
    add(w, leave(1), 1);   // 1-byte trailer
    add(w, 33, 1);
  }
  L.img = sink.contents;
  return L;
}

// header offsets of the physical records of an intact image: walk as log_reader.cc does
std::vector<uint64_t> log_phys(const std::string& img) {
  std::vector<uint64_t> phys;
  for (uint64_t b = 0; b < img.size(); b += kBlock) {
    uint64_t p = b;
    const uint64_t end = std::min<uint64_t>(b + kBlock, img.size());
    while (end - p >= kHeader) {
      const uint64_t l = uint8_t(img[p + 4]) | (uint64_t(uint8_t(img[p + 5])) << 8);
      if (img[p + 6] == 0 && l == 0) break;
      phys.push_back(p);
      p += kHeader + l;
    }
  }
  return phys;
}

std::string log_section(const std::string& dir) {
  const LogImage L = build_log();
  const std::string& img = L.img;
  const std::vector<uint64_t>& lens = L.lens;
  const std::vector<int>& writer_of = L.writer_of;
  const uint64_t reopen_at = L.reopen_at;
  if (!dir.empty() && !write_file(dir + "/manifest.log", img)) std::abort();
  const std::vector<uint64_t> phys = log_phys(img);
  auto frag_len = [&](size_t k) { return uint8_t(img[phys[k] + 4]) | (uint64_t(uint8_t(img[phys[k] + 5])) << 8); };
  auto first_of_type = [&](int t, size_t from) {
    for (size_t k = from; k < phys.size(); ++k)
      if (img[phys[k] + 6] == t && frag_len(k) > 0) return k;
    std::abort();
  };
  const size_t full = first_of_type(1, 0), first = first_of_type(2, 0), middle = first_of_type(3, 0),
               last = first_of_type(4, middle);
  struct Case {
    const char* name;
    uint64_t flip;
  };
  const Case cases[] = {{"full_payload", phys[full] + kHeader + frag_len(full) / 2},
                        {"first_payload", phys[first] + kHeader + 17},
                        {"middle_payload", phys[middle] + kHeader + 1000},
                        {"last_payload", phys[last] + kHeader + frag_len(last) - 1},
                        {"type_byte", phys[middle] + 6},
                        {"length_field", phys[first_of_type(1, last)] + 5},
                        {"crc_after_reopen", phys[first_of_type(2, first_of_type(1, last))] + 2}};
  std::string cs = "[";
  for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c) {
    std::string bad = img;
    bad[cases[c].flip] ^= char(0x80);
    char b[128];
    std::snprintf(b, sizeof b, "%s{\"name\":\"%s\",\"flip\":%llu,\"reader\":", c ? "," : "", cases[c].name,
                  (unsigned long long)cases[c].flip);
    cs += b + log_read(bad) + "}";
  }
  cs += "]";
  std::string ls = "[", ws = "[";
  for (size_t i = 0; i < lens.size(); ++i) {
    ls += (i ? "," : "") + std::to_string(lens[i]);
    ws += (i ? "," : "") + std::to_string(writer_of[i]);
  }
  return "{\"seed\":" + std::to_string(kLogSeed) + ",\"lens\":" + ls + "],\"writer\":" + ws +
         "],\"reopen_at\":" + std::to_string(reopen_at) + ",\"size\":" + std::to_string(img.size()) +
         ",\"physical_records\":" + std::to_string(phys.size()) + ",\"intact\":" + log_read(img) + ",\"cases\":" + cs +
         "}";
}

// ------------------------------------------------------------------ SST
constexpr uint64_t kSstSeed = 0x73737462;

typedef std::vector<std::pair<uint64_t, uint64_t>> SstBlocks;  // (offset, size) of every block

std::string build_sst(SstBlocks* blocks) {
  leveldb::Options opt;  // block_size 4 KiB (include/leveldb/options.h:101); no snappy here -> raw blocks
  opt.compression = leveldb::kNoCompression;
  StringSink sink;
  {
    leveldb::TableBuilder tb(opt, &sink);
    for (int i = 0; i < 1500; ++i) {
      char key[32];
      std::snprintf(key, sizeof key, "key%08d", i * 7);
      const std::string v = stream_bytes(kSstSeed, uint64_t(i) * 100, 37 + (i * 13) % 200);
      tb.Add(Slice(key), Slice(v));
    }
    if (!tb.Finish().ok()) std::abort();
  }
  // WriteRawBlock appends the block, then its 5-byte trailer (table/table_builder.cc:217-227): every Append
  // followed by a 5-byte Append is a block.
  for (size_t i = 0; i + 1 < sink.appends.size(); ++i)
    if (sink.appends[i + 1].second == leveldb::kBlockTrailerSize &&
        sink.appends[i + 1].first == sink.appends[i].first + sink.appends[i].second)
      blocks->push_back(sink.appends[i]);
  return sink.contents;
}

// ReadBlock(verify_checksums) per block: 1 = ok
std::vector<int> sst_verdicts(const std::string& f, const SstBlocks& blocks) {
  StringRandom file(f);
  leveldb::ReadOptions ro;
  ro.verify_checksums = true;
  std::vector<int> v;
  for (size_t k = 0; k < blocks.size(); ++k) {
    leveldb::BlockHandle h;
    h.set_offset(blocks[k].first);
    h.set_size(blocks[k].second);
    leveldb::BlockContents bc;
    const Status st = leveldb::ReadBlock(&file, ro, h, &bc);
    if (st.ok() && bc.heap_allocated) delete[] bc.data.data();
    v.push_back(st.ok() ? 1 : 0);
  }
  return v;
}

std::string sst_section(const std::string& dir) {
  SstBlocks blocks;
  const std::string img = build_sst(&blocks);
  if (!dir.empty() && !write_file(dir + "/table.sst", img)) std::abort();
  auto verdicts = [&](const std::string& f) {
    std::string s = "[";
    const std::vector<int> v = sst_verdicts(f, blocks);
    for (size_t k = 0; k < v.size(); ++k) s += std::string(k ? "," : "") + (v[k] ? "1" : "0");
    return s + "]";
  };
  std::string bl = "[";
  for (size_t k = 0; k < blocks.size(); ++k) {
    const uint64_t o = blocks[k].first, n = blocks[k].second;
    bl += (k ? ",[" : "[") + std::to_string(o) + "," + std::to_string(n) + "," + std::to_string(uint8_t(img[o + n])) +
          ",\"" + hex(&img[o + n + 1], 4) + "\"]";
  }
  bl += "]";
  const uint64_t b5 = blocks[5].first, b9 = blocks[9].first + blocks[9].second, b2 = blocks[2].first + blocks[2].second,
                 bi = blocks.back().first;
  const uint64_t flips[] = {b5 + 100, b9 + 3, b2, bi + 1};
  const char* names[] = {"data_block_5", "trailer_crc_9", "type_byte_2", "last_block"};
  std::string cs = "[";
  for (int c = 0; c < 4; ++c) {
    std::string bad = img;
    bad[flips[c]] ^= char(0x80);
    cs += std::string(c ? "," : "") + "{\"name\":\"" + names[c] + "\",\"flip\":" + std::to_string(flips[c]) +
          ",\"ok\":" + verdicts(bad) + "}";
  }
  cs += "]";
  return "{\"size\":" + std::to_string(img.size()) + ",\"blocks\":" + bl + ",\"intact_ok\":" + verdicts(img) +
         ",\"cases\":" + cs + "}";
}

// ------------------------------------------------------------------ corpus of damaged files
// `corpus` mode: a deterministic list of mutations of the three base images, each read back by the reference's own
// reader.  tests/golden/make_framing_corpus.py commits the mutations and what the readers returned and reported;
// tests/test_framing_reference_cpu.py and tests/test_gpu_framing_corpus.py replay them through the library.
//
// A mutation is applied in this order: cut the image to `cut` bytes (if >= 0), append `append` zero bytes, fill
// [pos, pos + len) with one byte (`fills`), then write single bytes (`writes`).  A mutant that needs a valid checksum
// over altered bytes (a retyped fragment) is restamped here with the reference's crc32c and carries the resulting
// bytes as plain writes.
struct Mutation {
  std::string cls, name;
  int64_t cut = -1;
  uint64_t append = 0;
  std::vector<std::array<uint64_t, 3>> fills;  // pos, len, byte
  std::vector<std::pair<uint64_t, uint8_t>> writes;
};

std::string apply(const std::string& base, const Mutation& m) {
  std::string s = base;
  if (m.cut >= 0) {
    if (uint64_t(m.cut) > s.size()) std::abort();
    s.resize(size_t(m.cut));
  }
  s.append(m.append, '\0');
  for (const auto& f : m.fills) {
    if (f[0] + f[1] > s.size()) std::abort();
    std::memset(&s[f[0]], int(f[2]), f[1]);
  }
  for (const auto& w : m.writes) {
    if (w.first >= s.size()) std::abort();
    s[w.first] = char(w.second);
  }
  return s;
}

std::string mutation_json(const Mutation& m) {
  std::string s = "\"class\":\"" + m.cls + "\",\"name\":\"" + m.name + "\",\"cut\":" +
                  (m.cut < 0 ? std::string("null") : std::to_string(m.cut)) + ",\"append\":" + std::to_string(m.append) +
                  ",\"fills\":[";
  for (size_t i = 0; i < m.fills.size(); ++i)
    s += std::string(i ? "," : "") + "[" + std::to_string(m.fills[i][0]) + "," + std::to_string(m.fills[i][1]) + "," +
         std::to_string(m.fills[i][2]) + "]";
  s += "],\"writes\":[";
  for (size_t i = 0; i < m.writes.size(); ++i)
    s += std::string(i ? "," : "") + "[" + std::to_string(m.writes[i].first) + "," + std::to_string(m.writes[i].second) +
         "]";
  return s + "]";
}

struct Rng {  // the repo's splitmix64 stream as a counter-based generator
  uint64_t seed, n;
  uint64_t next() { return splitmix_word(seed, n++); }
  uint64_t below(uint64_t k) { return next() % k; }
};

void flip(Mutation& m, const std::string& base, uint64_t pos, uint8_t x = 0x80) {
  m.writes.emplace_back(pos, uint8_t(uint8_t(base[pos]) ^ x));
}

void put32(Mutation& m, uint64_t pos, uint32_t v) {
  for (int i = 0; i < 4; ++i) m.writes.emplace_back(pos + i, uint8_t(v >> (8 * i)));
}

Mutation mut(const std::string& cls, const std::string& name) {
  Mutation m;
  m.cls = cls;
  m.name = name;
  return m;
}

// ---- log
struct Phys {
  uint64_t pos, len;
  int type;
  bool first, last;  // of its 32 KiB block
};

std::vector<Phys> log_phys_info(const std::string& img) {
  const std::vector<uint64_t> at = log_phys(img);
  std::vector<Phys> v;
  for (size_t k = 0; k < at.size(); ++k) {
    const uint64_t p = at[k];
    v.push_back({p, uint8_t(img[p + 4]) | (uint64_t(uint8_t(img[p + 5])) << 8), uint8_t(img[p + 6]), p % kBlock == 0,
                 k + 1 == at.size() || at[k + 1] / kBlock != p / kBlock});
  }
  return v;
}

uint64_t block_end(uint64_t size, uint64_t pos) { return std::min<uint64_t>((pos / kBlock + 1) * kBlock, size); }

void set_len16(Mutation& m, uint64_t p, uint64_t v) {
  m.writes.emplace_back(p + 4, uint8_t(v));
  m.writes.emplace_back(p + 5, uint8_t(v >> 8));
}

// Stamp the header at p of the mutated image with Mask(Value(type || payload)) for the type and length it now holds
// (db/log_writer.cc:98-103), when that length still fits its block.
void restamp_log(Mutation& m, const std::string& base, uint64_t p) {
  const std::string img = apply(base, m);
  if (p + kHeader > img.size()) return;
  const uint64_t l = uint8_t(img[p + 4]) | (uint64_t(uint8_t(img[p + 5])) << 8);
  if (p + kHeader + l > block_end(img.size(), p)) return;
  put32(m, p, leveldb::crc32c::Mask(leveldb::crc32c::Value(&img[p + 6], 1 + l)));
}

const char* kind_of(const Phys& ph) {
  switch (ph.type) {
    case 1: return ph.len ? "FULL" : "FULL0";
    case 2: return ph.len ? "FIRST" : "FIRST0";
    case 3: return "MIDDLE";
    default: return "LAST";
  }
}

std::vector<Mutation> log_mutations(const LogImage& L) {
  const std::string& img = L.img;
  const uint64_t size = img.size();
  const std::vector<Phys> phys = log_phys_info(img);
  std::vector<Mutation> out;
  // representatives: each kind of physical record at the start, inside and at the end of a block, and after the
  // reopen point, where such a record exists
  std::vector<std::pair<std::string, Phys>> reps;
  const char* kinds[] = {"FULL", "FIRST", "MIDDLE", "LAST", "FIRST0", "FULL0"};
  const char* places[] = {"first", "inner", "last", "reopened"};
  for (const char* kind : kinds)
    for (int pl = 0; pl < 4; ++pl)
      for (const Phys& ph : phys) {
        const bool here = pl == 0 ? ph.first : pl == 1 ? !ph.first && !ph.last : pl == 2 ? ph.last : ph.pos >= L.reopen_at;
        if (!here || std::strcmp(kind_of(ph), kind)) continue;
        bool seen = false;
        for (const auto& r : reps) seen = seen || r.second.pos == ph.pos;
        if (!seen) reps.emplace_back(std::string(kind) + "." + places[pl] + "@" + std::to_string(ph.pos), ph);
        break;
      }
  for (const auto& r : reps) {
    const Phys& ph = r.second;
    const uint64_t p = ph.pos, rest = block_end(size, p) - p - kHeader;
    for (int i = 0; i < 4; ++i) {
      Mutation m = mut("log_crc", r.first + " crc byte " + std::to_string(i));
      flip(m, img, p + i);
      out.push_back(m);
    }
    if (ph.len) {
      Mutation m = mut("log_payload", r.first + " first payload byte");
      flip(m, img, p + kHeader);
      out.push_back(m);
      if (ph.len > 1) {
        m = mut("log_payload", r.first + " last payload byte");
        flip(m, img, p + kHeader + ph.len - 1);
        out.push_back(m);
      }
    }
    const std::pair<const char*, uint64_t> lens[] = {{"len+1", ph.len + 1}, {"len-1", ph.len ? ph.len - 1 : ph.len},
                                                     {"0", 0},              {"rest of block", rest},
                                                     {"rest of block+1", rest + 1}, {"0xffff", 0xffff}};
    std::vector<uint64_t> done{ph.len};
    for (const auto& lv : lens) {
      if (std::find(done.begin(), done.end(), lv.second) != done.end()) continue;
      done.push_back(lv.second);
      Mutation m = mut("log_length", r.first + " length " + lv.first);
      set_len16(m, p, lv.second);
      out.push_back(m);
    }
    for (int restamped = 0; restamped < 2; ++restamped)
      for (int t : {0, 5, 6, 255, 1, 2, 3, 4}) {  // 5 and 6 are the reader's own kEof / kBadRecord codes
        if (t == ph.type) continue;
        Mutation m = mut(restamped ? "log_type_restamped" : "log_type_stale", r.first + " type " + std::to_string(t));
        m.writes.emplace_back(p + 6, uint8_t(t));
        if (restamped) restamp_log(m, img, p);
        out.push_back(m);
      }
    Mutation z = mut("log_zero_header", r.first + " header zeroed");
    z.fills.push_back({p, kHeader, 0});
    out.push_back(z);
  }
  // chain gaps: a block dropped by its first header (zeroed, or a length past the block end) between the fragments
  // of a record
  const uint64_t nblk = (size + kBlock - 1) / kBlock;
  std::vector<int> first_type(nblk, 0);
  std::vector<bool> has_first(nblk, false);
  for (const Phys& ph : phys) {
    if (ph.first) first_type[ph.pos / kBlock] = ph.type;
    if (ph.type == 2) has_first[ph.pos / kBlock] = true;
  }
  auto damage = [&](Mutation& m, uint64_t b, int mode) {
    if (mode == 0) m.fills.push_back({b * kBlock, kHeader, 0});
    else set_len16(m, b * kBlock, 0xffff);
  };
  const char* modes[] = {"first header zeroed", "first header length 0xffff"};
  for (int mode = 0; mode < 2; ++mode)
    for (uint64_t b = 0; b < nblk; ++b) {
      if (first_type[b] == 3) {
        Mutation m = mut("log_chain_gap", "middle block " + std::to_string(b) + ": " + modes[mode]);
        damage(m, b, mode);
        out.push_back(m);
        if (b + 1 < nblk) {
          m = mut("log_chain_gap", "blocks " + std::to_string(b) + " and " + std::to_string(b + 1) + ": " + modes[mode]);
          damage(m, b, mode);
          damage(m, b + 1, mode);
          out.push_back(m);
        }
      }
      if (first_type[b] == 4 && has_first[b]) {
        Mutation m = mut("log_chain_gap", "LAST+FIRST block " + std::to_string(b) + ": " + modes[mode]);
        damage(m, b, mode);
        out.push_back(m);
      }
    }
  for (uint64_t b = 0; b < nblk; ++b)
    if (first_type[b] == 3 || first_type[b] == 4) {
      Mutation m = mut("log_chain_gap", "block " + std::to_string(b) + " replaced with zeros");
      m.fills.push_back({b * kBlock, block_end(size, b * kBlock) - b * kBlock, 0});
      out.push_back(m);
    }
  // truncation and padding
  std::vector<uint64_t> cuts;
  auto cut_at = [&](uint64_t c, const std::string& what) {
    if (c > size || std::find(cuts.begin(), cuts.end(), c) != cuts.end()) return;
    cuts.push_back(c);
    Mutation m = mut("log_truncate_pad", "cut at " + std::to_string(c) + ": " + what);
    m.cut = int64_t(c);
    out.push_back(m);
  };
  for (uint64_t k = 1; k * kBlock <= size; ++k) {  // a cut AT a boundary leaves a last block that was read in full
    cut_at(k * kBlock - 1, "block boundary - 1");
    cut_at(k * kBlock, "block boundary");
    cut_at(k * kBlock + 1, "block boundary + 1");
  }
  std::vector<Phys> heads{phys[1], phys.back()};
  for (const Phys& ph : phys)
    if (ph.first && ph.type == 3) {
      heads.push_back(ph);
      break;
    }
  for (const Phys& ph : heads) {
    for (uint64_t k = 1; k < kHeader; ++k) cut_at(ph.pos + k, std::to_string(k) + " header bytes");
    if (ph.len) cut_at(ph.pos + kHeader, "a whole header, no payload");
  }
  for (const char* kind : {"FULL", "FIRST", "MIDDLE", "LAST"})
    for (const Phys& ph : phys)
      if (!std::strcmp(kind_of(ph), kind)) {
        cut_at(ph.pos + kHeader + ph.len / 2, std::string("mid-payload of a ") + kind);
        break;
      }
  for (const Phys& ph : phys) {
    const uint64_t end = block_end(size, ph.pos), trailer = end - (ph.pos + kHeader + ph.len);
    if (ph.last && end % kBlock == 0 && trailer)
      for (uint64_t k = 1; k <= trailer; ++k) cut_at(end - k, "inside a " + std::to_string(trailer) + "-byte trailer");
  }
  for (uint64_t k : {uint64_t(2), uint64_t(5)})  // a bad length in the last block: reported only if it was read in full
    for (uint64_t less : {uint64_t(0), uint64_t(1)}) {
      Mutation m = mut("log_truncate_pad", "cut at " + std::to_string(k * kBlock - less) + " with the last block's first " +
                                               "header length 0xffff");
      m.cut = int64_t(k * kBlock - less);
      set_len16(m, (k - 1) * kBlock, 0xffff);
      out.push_back(m);
    }
  for (uint64_t z : {uint64_t(1), uint64_t(6), uint64_t(7), uint64_t(40), uint64_t(32768)}) {
    Mutation m = mut("log_truncate_pad", std::to_string(z) + " zero bytes appended");
    m.append = z;
    out.push_back(m);
  }
  // random: 1-4 writes (half of them aimed at a header) and an optional cut; headers hit in their length or type
  // byte are restamped half of the time so that the damage gets past the checksum
  Rng rng{0x6c6f6772616e64ull, 0};
  for (int i = 0; i < 200; ++i) {
    char name[16];
    std::snprintf(name, sizeof name, "r%03d", i);
    Mutation m = mut("log_random", name);
    uint64_t cur = size;
    if (rng.below(4) == 0) {
      cur = rng.below(size + 1);
      m.cut = int64_t(cur);
    }
    const uint64_t nw = 1 + rng.below(4);
    std::vector<uint64_t> stamp;
    for (uint64_t w = 0; w < nw && cur; ++w) {
      uint64_t pos;
      if (rng.below(2)) {
        const Phys& ph = phys[rng.below(phys.size())];
        const uint64_t k = rng.below(kHeader);
        pos = ph.pos + k;
        if (pos < cur && k >= 4 && rng.below(2)) stamp.push_back(ph.pos);
      } else {
        pos = rng.below(cur);
      }
      if (pos >= cur) pos = rng.below(cur);
      m.writes.emplace_back(pos, uint8_t(uint8_t(img[pos]) ^ (1 + rng.below(255))));
    }
    for (uint64_t p : stamp) restamp_log(m, img, p);
    out.push_back(m);
  }
  return out;
}

// ---- vlog
const uint64_t kSmallVlogLens[] = {0, 1, 7, 8, 15, 16, 100, 4095, 4096, 65539, 33};
constexpr size_t kSmallVlogN = sizeof(kSmallVlogLens) / sizeof(kSmallVlogLens[0]);
constexpr uint64_t kVlogLenCap = 16u << 20;  // VlogReader allocates `length` bytes before it reads

uint32_t get32(const std::string& s, uint64_t p) {
  return uint8_t(s[p]) | (uint32_t(uint8_t(s[p + 1])) << 8) | (uint32_t(uint8_t(s[p + 2])) << 16) |
         (uint32_t(uint8_t(s[p + 3])) << 24);
}

bool vlog_lengths_capped(const std::string& img) {  // every length field the reader gets to (it stops at a mismatch)
  uint64_t p = 0;
  while (p + 8 <= img.size()) {
    const uint64_t l = get32(img, p + 4);
    if (l >= kVlogLenCap) return false;
    if (l > img.size() - p - 8) break;
    if (leveldb::crc32c::Mask(leveldb::crc32c::Value(&img[p + 8], l)) != get32(img, p)) break;
    p += 8 + l;
  }
  return true;
}

std::vector<Mutation> vlog_mutations(const std::string& img) {
  const uint64_t size = img.size();
  std::vector<uint64_t> at;
  for (uint64_t i = 0, p = 0; i < kSmallVlogN; p += 8 + kSmallVlogLens[i], ++i) at.push_back(p);
  std::vector<Mutation> out;
  for (size_t r : {size_t(0), size_t(1), size_t(9), kSmallVlogN - 1}) {  // first (0-length), 1 byte, 65539 bytes, last
    const uint64_t p = at[r], len = kSmallVlogLens[r], rest = size - p - 8;
    const std::string who = "record " + std::to_string(r) + " (" + std::to_string(len) + " B)";
    for (int i = 0; i < 4; ++i) {
      Mutation m = mut("vlog_crc", who + " crc byte " + std::to_string(i));
      flip(m, img, p + i);
      out.push_back(m);
    }
    if (len) {
      Mutation m = mut("vlog_payload", who + " first payload byte");
      flip(m, img, p + 8);
      out.push_back(m);
      if (len > 1) {
        m = mut("vlog_payload", who + " last payload byte");
        flip(m, img, p + 8 + len - 1);
        out.push_back(m);
      }
    }
    const std::pair<const char*, uint64_t> lens[] = {{"len+1", len + 1}, {"len-1", len ? len - 1 : len}, {"0", 0},
                                                     {"rest of file", rest}, {"rest of file+1", rest + 1}};
    std::vector<uint64_t> done{len};
    for (const auto& lv : lens) {
      if (std::find(done.begin(), done.end(), lv.second) != done.end()) continue;
      done.push_back(lv.second);
      Mutation m = mut("vlog_length", who + " length " + lv.first);
      put32(m, p + 4, uint32_t(lv.second));
      out.push_back(m);
    }
    std::vector<uint64_t> cuts;
    for (uint64_t k = 0; k < 8; ++k) cuts.push_back(p + k);
    if (len > 1) cuts.push_back(p + 8 + len / 2);
    for (uint64_t c : cuts) {
      Mutation m = mut("vlog_cut", who + " cut after " + std::to_string(c - p) + " of its bytes");
      m.cut = int64_t(c);
      out.push_back(m);
    }
  }
  for (uint64_t k = 1; k <= 7; ++k) {
    Mutation m = mut("vlog_append", std::to_string(k) + " junk bytes appended");
    m.append = k;
    for (uint64_t i = 0; i < k; ++i) m.writes.emplace_back(size + i, uint8_t(0xa5 + 17 * i));
    out.push_back(m);
  }
  for (uint64_t z : {uint64_t(8), uint64_t(16)}) {  // a zero header: a 0-length record whose stored word is not Mask(0)
    Mutation m = mut("vlog_append", std::to_string(z) + " zero bytes appended");
    m.append = z;
    out.push_back(m);
  }
  Rng rng{0x766c6f6772616e64ull, 0};
  for (int i = 0; i < 200;) {
    char name[16];
    std::snprintf(name, sizeof name, "r%03d", i);
    Mutation m = mut("vlog_random", name);
    uint64_t cur = size;
    if (rng.below(4) == 0) {
      cur = rng.below(size + 1);
      m.cut = int64_t(cur);
    }
    const uint64_t nw = 1 + rng.below(4);
    for (uint64_t w = 0; w < nw && cur; ++w) {
      uint64_t pos = rng.below(2) ? at[rng.below(at.size())] + rng.below(8) : rng.below(cur);
      if (pos >= cur) pos = rng.below(cur);
      m.writes.emplace_back(pos, uint8_t(uint8_t(img[pos]) ^ (1 + rng.below(255))));
    }
    if (!vlog_lengths_capped(apply(img, m))) continue;  // draw another one
    out.push_back(m);
    ++i;
  }
  for (const Mutation& m : out)
    if (!vlog_lengths_capped(apply(img, m))) std::abort();
  return out;
}

// ---- SST: every damaged byte leaves the checksum stale, so ReadBlock never reaches decompression
std::vector<Mutation> sst_mutations(const std::string& img, const SstBlocks& blocks) {
  std::vector<Mutation> out;
  const size_t nb = blocks.size();
  for (size_t b : {size_t(0), size_t(7), nb / 2, nb - 1}) {  // three data blocks and the last (index) block
    const uint64_t o = blocks[b].first, n = blocks[b].second;
    for (uint64_t k = 0; k < 5; ++k) {
      Mutation m = mut("sst_trailer", "block " + std::to_string(b) + " trailer byte " + std::to_string(k));
      flip(m, img, o + n + k);
      out.push_back(m);
    }
    Mutation m = mut("sst_block_byte", "block " + std::to_string(b) + " first byte");
    flip(m, img, o);
    out.push_back(m);
    m = mut("sst_block_byte", "block " + std::to_string(b) + " last byte");
    flip(m, img, o + n - 1);
    out.push_back(m);
  }
  Rng rng{0x73737472616e64ull, 0};
  for (size_t k : {size_t(2), size_t(9), nb}) {
    std::vector<size_t> pick;
    while (pick.size() < k) {
      const size_t b = rng.below(nb);
      if (std::find(pick.begin(), pick.end(), b) == pick.end()) pick.push_back(b);
    }
    Mutation m = mut("sst_multi", std::to_string(k) + " blocks damaged");
    for (size_t b : pick) flip(m, img, blocks[b].first + rng.below(blocks[b].second + 5), uint8_t(1 + rng.below(255)));
    out.push_back(m);
  }
  for (int i = 0; i < 200; ++i) {  // no cuts: a handle past the end of the image is refused by the library's contract
    char name[16];
    std::snprintf(name, sizeof name, "r%03d", i);
    Mutation m = mut("sst_random", name);
    const uint64_t nw = 1 + rng.below(4);
    for (uint64_t w = 0; w < nw; ++w) {
      const uint64_t pos = rng.below(img.size());
      m.writes.emplace_back(pos, uint8_t(uint8_t(img[pos]) ^ (1 + rng.below(255))));
    }
    out.push_back(m);
  }
  return out;
}

std::string corpus(const std::string& dir) {
  const LogImage L = build_log();
  if (!dir.empty() && !write_file(dir + "/manifest.log", L.img)) std::abort();  // the bases, for the generator to
  std::string lj = "{\"size\":" + std::to_string(L.img.size()) + ",\"reopen_at\":" + std::to_string(L.reopen_at) +
                   ",\"intact\":" + log_read(L.img) + ",\"mutants\":[";
  bool sep = false;
  for (const Mutation& m : log_mutations(L)) {
    lj += std::string(sep ? ",\n" : "\n") + "{" + mutation_json(m) + ",\"reader\":" + log_read(apply(L.img, m)) + "}";
    sep = true;
  }
  lj += "]}";

  const std::string vimg = build_vlog(kSmallVlogLens, kSmallVlogN, nullptr);
  if (!dir.empty() && !write_file(dir + "/small_vlog.bin", vimg)) std::abort();
  std::string vj = "{\"seed\":" + std::to_string(kVlogSeed) + ",\"lens\":[";
  for (size_t i = 0; i < kSmallVlogN; ++i) vj += (i ? "," : "") + std::to_string(kSmallVlogLens[i]);
  vj += "],\"size\":" + std::to_string(vimg.size()) + ",\"intact\":" + vlog_read(vimg) + ",\"mutants\":[";
  sep = false;
  for (const Mutation& m : vlog_mutations(vimg)) {
    vj += std::string(sep ? ",\n" : "\n") + "{" + mutation_json(m) + ",\"reader\":" + vlog_read(apply(vimg, m)) + "}";
    sep = true;
  }
  vj += "]}";

  SstBlocks blocks;
  const std::string simg = build_sst(&blocks);
  if (!dir.empty() && !write_file(dir + "/table.sst", simg)) std::abort();  // compare with the committed fixtures
  auto bad_json = [&](const std::string& f) {  // the blocks ReadBlock rejects, by index
    std::string s = "[";
    const std::vector<int> v = sst_verdicts(f, blocks);
    for (size_t k = 0; k < v.size(); ++k)
      if (!v[k]) s += (s.size() > 1 ? "," : "") + std::to_string(k);
    return s + "]";
  };
  std::string sj = "{\"size\":" + std::to_string(simg.size()) + ",\"blocks\":[";
  for (size_t k = 0; k < blocks.size(); ++k)
    sj += std::string(k ? "," : "") + "[" + std::to_string(blocks[k].first) + "," + std::to_string(blocks[k].second) + "]";
  sj += "],\"intact_bad\":" + bad_json(simg) + ",\"mutants\":[";
  sep = false;
  for (const Mutation& m : sst_mutations(simg, blocks)) {
    sj += std::string(sep ? ",\n" : "\n") + "{" + mutation_json(m) + ",\"bad\":" + bad_json(apply(simg, m)) + "}";
    sep = true;
  }
  sj += "]}";
  return "{\"log\":" + lj + ",\n\"vlog\":" + vj + ",\n\"sst\":" + sj + "}";
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "corpus") == 0) {  // <binary> corpus [out_dir]
    std::printf("%s\n", corpus(argc > 2 ? argv[2] : "").c_str());
    return 0;
  }
  const std::string dir = argc > 1 ? argv[1] : "";
  const bool gpu = argc > 2 && std::strcmp(argv[2], "gpu") == 0;
#ifdef KVSEP_CALLSITE
  if (gpu) {  // every Extend of the reference call sites on the GPU
    kvsep_set_offload_threshold(0);
    kvsep_set_offload_wait(1);
  }
#else
  if (gpu) {
    std::fprintf(stderr, "gpu mode needs the KVSEP_CALLSITE build\n");
    return 2;
  }
#endif
  const std::string j = "{\"vlog\":" + vlog_section(dir) + ",\"log\":" + log_section(dir) + ",\"sst\":" +
                        sst_section(dir) + "}";
#ifdef KVSEP_CALLSITE
  uint64_t g = 0, h = 0, f = 0;
  kvsep_offload_stats(&g, &h, &f);
  std::fprintf(stderr, "kvsep offload: %llu gpu calls, %llu host calls, %llu gpu failures\n", (unsigned long long)g,
               (unsigned long long)h, (unsigned long long)f);
  if (gpu && (g == 0 || h != 0 || f != 0)) return 3;  // every call must have run on the GPU
#endif
  std::printf("%s\n", j.c_str());
  return 0;
}
