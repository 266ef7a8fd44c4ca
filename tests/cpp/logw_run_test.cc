// logw_run_test.cc -- the rules of the log / MANIFEST write side (csrc/logw_run.h) on the CPU, no GPU and no library.
//
// emulate() below is the control flow of the two kernels of csrc/crc32c_logframe.inc written lane by lane over a memory
// model: logw_layout_kernel's one wavefront (rows loaded ahead, the 32-bit DPP scan step by step, the reset ballot, the
// commit and rescan loop, the two 64-bit scans, rows chained) and logw_fill_kernel's lane per fragment slot and per
// record (owner search, descriptors, seeds, padding, pad zeros).  The copy that follows them on the stream is reduced
// to what it decides from their outputs: pack::fits and pack::log_header_byte per slot (tests/cpp/pack_run_test.cc runs
// the copy itself); the "checksum" of a fragment is its seed, so the model needs no CRC.  Every decision is a call into
// logw_run.h, the header the kernels and kvsep_log_frame_layout include.  Per emulated call:
//   * rec_at / frag_first / the five fragment arrays / *nfrag / *written, and where asked the bytes of dst, equal
//     log::Writer::AddRecord's loop (db/log_writer.cc:35-82) restated serially, fragment by fragment (reference());
//   * every output element is written exactly once -- rec_at for count, frag_first for count + 1, the fragment arrays
//     for frag_cap -- and nothing around them; no byte of dst at or past *written or outside [0, dst_bytes);
//   * len / keep are read below count only, off only for a record that is laid out, the source only inside it;
//   * every scratch word read was written earlier in the same call.
// Three deliberately wrong rules must each be caught.  Built with -fsanitize=address,undefined by
// tests/test_logw_run_cpu.py and run as it is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "logw_run.h"
#include "pack_run.h"

using namespace kvsep;

namespace {

constexpr uint64_t kCanary = 0xC0FFEE1234567ull;
constexpr uint64_t kGuard = 3;     // canary elements on each side of every output
constexpr uint64_t kDstGuard = 16;  // canary bytes on each side of dst
constexpr uint64_t kBig = uint64_t(1) << 40;  // a length the serial loop does not walk fragment by fragment

long g_failed = 0, g_cases = 0;
std::string g_case;

struct Call {
  std::vector<uint64_t> len, off;
  std::vector<uint8_t> keep;  // empty: no mask
  uint64_t dest_length = 0, frag_cap = 0, dst_bytes = 0;
  bool bytes = false;  // also build and compare dst
  uint64_t count() const { return len.size(); }
  bool kept(uint64_t i) const { return keep.empty() || keep[i] != 0; }
};

struct Rules {
  bool eager_pad = false;      // wrong: the trailer is charged to the record that leaves it
  bool seven_is_pad = false;   // wrong: a leftover of exactly 7 bytes is zero-filled
  bool no_rescan = false;      // wrong: a row is committed whole although a record in it leaves a reset
};

// ---- log::Writer::AddRecord restated: one number, fragment by fragment
struct Phys {
  uint64_t at, src, len;
  uint8_t type;
};
struct Want {
  std::vector<uint64_t> rec_at, frag_first;
  std::vector<Phys> phys;
  std::vector<std::pair<uint64_t, uint64_t>> pads;  // [at, at + n) zero
  uint64_t nfrag = 0, written = 0;
};

Want reference(const Call& c) {
  Want w;
  const uint64_t kBlk = 32768, kHdr = 7;
  const uint64_t b0 = c.dest_length % kBlk;
  unsigned __int128 pos = b0;  // the exact position, counted from the start of the log's current block
  uint64_t block_offset = b0;
  bool saturated = false;
  const unsigned __int128 kMaxBlock = (~uint64_t(0) - kBlk) / kBlk;  // logw::pos_sat's bound on the block index
  for (uint64_t r = 0; r < c.count(); ++r) {
    w.frag_first.push_back(w.phys.size());
    if (!c.kept(r)) {
      w.rec_at.push_back(~uint64_t(0));
      continue;
    }
    uint64_t left = c.len[r], src = c.len[r] < kBig ? c.off[r] : 0;
    if (c.len[r] >= kBig || saturated) {
      // not walked: only where it ends matters (these cases end past 2^64 - 1, or lie behind a record that does)
      uint64_t lo = kBlk - block_offset;
      if (lo < kHdr) pos += lo, block_offset = 0;
      const uint64_t first = kBlk - block_offset - kHdr;
      const unsigned __int128 nf = left <= first ? 1 : 2 + (unsigned __int128)(left - first - 1) / (kBlk - kHdr);
      pos += nf * kHdr + left;
      block_offset = left <= first ? block_offset + kHdr + left : kHdr + (left - first - 1) % (kBlk - kHdr) + 1;
      const unsigned __int128 blk = (pos - block_offset) / kBlk;
      if (blk > kMaxBlock) saturated = true;
      if (!saturated) {
        printf("FAILED %s: the reference walks no record this long that is laid out\n", g_case.c_str());
        ++g_failed;
      }
      w.rec_at.push_back(~uint64_t(0));
      continue;
    }
    bool begin = true;
    do {
      const uint64_t leftover = kBlk - block_offset;
      if (leftover < kHdr) {
        if (leftover) w.pads.emplace_back(uint64_t(pos) - b0, leftover);
        pos += leftover;
        block_offset = 0;
      }
      const uint64_t avail = kBlk - block_offset - kHdr;
      const uint64_t frag = left < avail ? left : avail;
      const bool end = left == frag;
      const uint8_t type = begin && end ? 1 : begin ? 2 : end ? 4 : 3;
      if (begin) w.rec_at.push_back(uint64_t(pos) - b0);
      w.phys.push_back({uint64_t(pos) - b0, src, frag, type});
      pos += kHdr + frag;
      block_offset += kHdr + frag;
      src += frag;
      left -= frag;
      begin = false;
    } while (left > 0);
  }
  w.frag_first.push_back(w.phys.size());
  w.nfrag = w.phys.size();
  w.written = saturated ? ~uint64_t(0) : uint64_t(pos - b0);
  return w;
}

// ---- the memory model
struct Word {
  uint32_t v = 0;
  bool set = false;
};

template <typename T>
struct Out {
  std::vector<T> v;
  std::vector<uint8_t> writes;
  uint64_t n;
  explicit Out(uint64_t n_) : v(n_ + 2 * kGuard, T(kCanary)), writes(n_ + 2 * kGuard, 0), n(n_) {}
  T at(uint64_t i) const { return v[kGuard + i]; }
};

constexpr uint32_t kSeed[5] = {0, 0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u};

struct Model {
  const Call& c;
  const std::vector<uint8_t>& base;
  long problems = 0;
  bool quiet;
  Out<uint64_t> rec_at, frag_first, frag_off, frag_len, frag_at;
  Out<uint8_t> frag_type;
  Out<uint32_t> frag_crc;
  uint64_t nfrag = kCanary, written = kCanary;
  int nfrag_writes = 0, written_writes = 0;
  std::vector<Word> rec, seed;
  std::vector<uint8_t> dst, dst_writes;

  Model(const Call& call, const std::vector<uint8_t>& b, bool q)
      : c(call), base(b), quiet(q), rec_at(call.count()), frag_first(call.count() + 1), frag_off(call.frag_cap),
        frag_len(call.frag_cap), frag_at(call.frag_cap), frag_type(call.frag_cap), frag_crc(call.frag_cap),
        rec(call.count()), seed(call.frag_cap) {
    if (c.bytes) dst.assign(c.dst_bytes + 2 * kDstGuard, 0xA5), dst_writes.assign(dst.size(), 0);
  }
  void bad(const char* what, uint64_t x = 0, uint64_t y = 0) {
    if (!quiet && g_failed + problems < 20)
      printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)x, (unsigned long long)y);
    ++problems;
  }
  uint64_t len_at(uint64_t i) {
    if (i >= c.count()) { bad("len[] read at or past count", i); return 0; }
    return c.len[i];
  }
  uint8_t keep_at(uint64_t i) {
    if (i >= c.count()) { bad("keep[] read at or past count", i); return 0; }
    return c.keep.empty() ? uint8_t(1) : c.keep[i];
  }
  uint64_t off_at(uint64_t i) {
    if (i >= c.count() || !c.kept(i)) { bad("off[] of a dropped record, or past count, read", i); return 0; }
    return c.off[i];
  }
  uint32_t rd(std::vector<Word>& a, uint64_t i, const char* what) {
    if (i >= a.size()) { bad(what, i); return 0; }
    if (!a[i].set) bad("a scratch word read before this call wrote it", i);
    return a[i].v;
  }
  void wr(std::vector<Word>& a, uint64_t i, uint32_t v, const char* what) {
    if (i >= a.size()) { bad(what, i); return; }
    a[i] = {v, true};
  }
  template <typename T>
  void put(Out<T>& o, uint64_t i, T v, const char* what) {
    if (i >= o.n) { bad(what, i); return; }
    o.v[kGuard + i] = v;
    ++o.writes[kGuard + i];
  }
  template <typename T>
  T get(Out<T>& o, uint64_t i, const char* what) {  // an output of the first kernel read by the second
    if (i >= o.n) { bad(what, i); return T(0); }
    if (!o.writes[kGuard + i]) bad("an output read before this call wrote it", i);
    return o.v[kGuard + i];
  }
  void st8(uint64_t at, uint8_t v) {
    if (!c.bytes) return;
    if (at >= c.dst_bytes) { bad("a byte stored outside [0, dst_bytes)", at); return; }
    dst[kDstGuard + at] = v;
    ++dst_writes[kDstGuard + at];
  }
};

uint64_t ballot(const bool (&b)[64]) {
  uint64_t m = 0;
  for (uint32_t l = 0; l < 64; ++l) m |= uint64_t(b[l]) << l;
  return m;
}

// the wave scans, step by step as the kernels run them (DPP row_shr within a 16-lane row, then the rows before)
void wave_scan(uint64_t (&v)[64]) {
  for (uint32_t step = 0; step < offsets::kScanSteps; ++step) {
    const uint32_t n = offsets::scan_shift(step);
    uint64_t left[64];
    for (uint32_t l = 0; l < 64; ++l) left[l] = (l & 15u) >= n ? v[l - n] : 0;
    for (uint32_t l = 0; l < 64; ++l) v[l] = offsets::add_sat(v[l], offsets::scan_takes(l, n) ? left[l] : 0);
  }
  const uint64_t t15 = v[15], t31 = v[31], t47 = v[47];
  for (uint32_t l = 0; l < 64; ++l) v[l] = offsets::add_sat(v[l], offsets::row_base(l, t15, t31, t47));
}

// logw:: as the kernels call it, or a wrong rule in its place
bool resets_of(const Rules& r, uint32_t raw) { return r.seven_is_pad ? raw >= logw::kAvail : logw::resets(raw); }
uint32_t start_of(const Rules& r, uint32_t raw) { return r.seven_is_pad ? (resets_of(r, raw) ? 0 : raw) : logw::start_of(raw); }
uint32_t pad_of(const Rules& r, uint32_t raw) {
  return r.seven_is_pad ? (resets_of(r, raw) ? logw::kBlock - raw : 0) : logw::pad_bytes(raw);
}
uint32_t raw_at(const Rules& r, uint32_t in, bool kept, uint32_t sum) {
  if (!r.seven_is_pad) return logw::raw_before(in, kept, sum);
  return kept ? logw::after(logw::join(start_of(r, in), sum)) : in;
}

void emulate_layout(Model& m, const Rules& rules) {
  const Call& c = m.c;
  const uint64_t count = c.count(), rows = logw::row_count(count);
  const uint32_t b0 = logw::start_state(c.dest_length);
  uint32_t r = b0;
  uint64_t block = 0, nfr = 0;
  for (uint64_t row = 0; row < rows; ++row) {
    uint64_t len[64] = {};
    bool own[64], kept[64];
    uint32_t x[64];
    for (uint32_t l = 0; l < 64; ++l) {
      const uint64_t i = row * logw::kWaveLanes + l;
      own[l] = i < count;
      kept[l] = false;
      if (own[l]) {
        len[l] = m.len_at(i);
        kept[l] = m.keep_at(i) != 0;
      }
      x[l] = logw::step_of(kept[l], len[l]);
    }
    const uint64_t km = ballot(kept);
    uint32_t rb[64] = {}, ra[64] = {};
    int turns = 0;
    for (uint64_t todo = ~uint64_t(0); todo;) {
      if (++turns > 65) { m.bad("the row loop does not end"); break; }
      uint64_t incl[64];
      for (uint32_t l = 0; l < 64; ++l) incl[l] = (todo >> l) & 1 ? x[l] : 0;
      wave_scan(incl);
      uint32_t before[64], behind[64];
      bool rs[64];
      for (uint32_t l = 0; l < 64; ++l) {
        const bool mine = (todo >> l) & 1;
        const uint32_t xs = mine ? x[l] : 0;
        const bool kb = (km & todo & logw::lanes_below(l)) != 0;
        before[l] = raw_at(rules, r, kb, uint32_t(incl[l]) - xs);
        behind[l] = raw_at(rules, r, kb || (mine && kept[l]), uint32_t(incl[l]));
        rs[l] = mine && kept[l] && resets_of(rules, behind[l]);
      }
      const uint64_t commit = rules.no_rescan ? todo : logw::commit_mask(todo, ballot(rs));
      if (!commit) { m.bad("a scan step commits no lane"); break; }
      for (uint32_t l = 0; l < 64; ++l)
        if ((commit >> l) & 1) rb[l] = before[l], ra[l] = behind[l];
      r = behind[logw::last_lane(commit)];
      todo &= ~commit;
    }
    uint64_t adv[64], fr[64], nf[64], bend[64];
    uint32_t b[64];
    bool is_laid[64];
    for (uint32_t l = 0; l < 64; ++l) {
      b[l] = start_of(rules, rb[l]);
      nf[l] = kept[l] ? logw::nfrag(b[l], len[l]) : 0;
      adv[l] = kept[l] ? logw::blocks_advanced(resets_of(rules, rb[l]), nf[l]) : 0;
    }
    wave_scan(adv);
    for (uint32_t l = 0; l < 64; ++l) {
      bend[l] = logw::add_sat(block, adv[l]);
      is_laid[l] = logw::laid(kept[l], bend[l], ra[l]);
      fr[l] = logw::frags_of(is_laid[l], nf[l]);
    }
    uint64_t fincl[64];
    for (uint32_t l = 0; l < 64; ++l) fincl[l] = fr[l];
    wave_scan(fincl);
    for (uint32_t l = 0; l < 64; ++l) {
      const uint64_t i = row * logw::kWaveLanes + l;
      if (!own[l]) continue;
      m.put(m.rec_at, i, logw::rec_at(is_laid[l], bend[l], nf[l], b[l], b0), "rec_at[] written at or past count");
      m.put(m.frag_first, i, logw::add_sat(nfr, fincl[l] - fr[l]), "frag_first[] written past count");
      m.wr(m.rec, i, logw::pack_rec(b[l], kept[l] ? pad_of(rules, rb[l]) : 0), "rec scratch written past count");
    }
    block = bend[63];
    nfr = logw::add_sat(nfr, fincl[63]);
  }
  m.put(m.frag_first, count, nfr, "frag_first[count]");
  m.nfrag = nfr, ++m.nfrag_writes;
  if (rules.eager_pad && logw::resets(r)) block = logw::add_sat(block, 1), r = 0;
  m.written = logw::rel(logw::pos_sat(block, r), b0), ++m.written_writes;
}

void emulate_fill(Model& m) {
  const Call& c = m.c;
  const uint64_t count = c.count(), lanes = logw::fill_lanes(count, c.frag_cap);
  for (uint64_t t = 0; t < lanes; ++t) {
    if (t < c.frag_cap) {
      const uint64_t nf = m.nfrag;
      if (logw::pads_frag(t, nf, c.frag_cap)) {
        m.put(m.frag_off, t, logw::kPadOff, "frag_off");
        m.put(m.frag_len, t, logw::kPadLen, "frag_len");
        m.put(m.frag_at, t, logw::kPadAt, "frag_at");
        m.put(m.frag_type, t, logw::kPadType, "frag_type");
        m.wr(m.seed, t, logw::kPadSeed, "seed");
      } else {
        if (!count) { m.bad("a fragment with no record"); continue; }
        const uint64_t i = logw::owner(t, count, [&](uint64_t j) {
          if (j >= count) m.bad("the owner search leaves [0, count)", j);
          return m.get(m.frag_first, j, "frag_first[] read past count");
        });
        const uint64_t k = t - m.get(m.frag_first, i, "frag_first");
        const uint32_t b = logw::rec_b(m.rd(m.rec, i, "rec scratch read past count"));
        const uint64_t len = m.len_at(i);
        const uint8_t type = logw::frag_type(k, logw::nfrag(b, len));
        m.put(m.frag_off, t, m.off_at(i) + logw::frag_begin(b, k), "frag_off");
        m.put(m.frag_len, t, logw::frag_len(b, len, k), "frag_len");
        m.put(m.frag_at, t, logw::frag_at(m.get(m.rec_at, i, "rec_at"), b, k), "frag_at");
        m.put(m.frag_type, t, type, "frag_type");
        m.wr(m.seed, t, logw::seed_of(type, kSeed[1], kSeed[2], kSeed[3], kSeed[4]), "seed");
      }
    }
    if (t < count) {
      const uint64_t at = m.get(m.rec_at, t, "rec_at");
      const uint32_t pad = logw::rec_pad(m.rd(m.rec, t, "rec scratch"));
      if (logw::writes_pad(at, pad, m.get(m.frag_first, t, "frag_first"), c.frag_cap, c.dst_bytes))
        for (uint32_t j = 0; j < pad; ++j) m.st8(at - pad + j, 0);
    }
  }
}

// What the checksum call and the copy take from the arrays: frag_crc = the seed (an empty Extend), and per slot the
// header and the bytes when the framed fragment lies inside the destination.
void emulate_copy(Model& m) {
  const Call& c = m.c;
  for (uint64_t f = 0; f < c.frag_cap; ++f) {
    m.put(m.frag_crc, f, m.rd(m.seed, f, "seed read past frag_cap"), "frag_crc");
    const uint64_t at = m.get(m.frag_at, f, "frag_at"), n = m.get(m.frag_len, f, "frag_len");
    if (!pack::fits(at, n, pack::kLog, c.dst_bytes)) continue;
    const uint64_t src = m.get(m.frag_off, f, "frag_off");
    for (uint32_t i = 0; i < pack::lead(pack::kLog); ++i)
      m.st8(at + i, pack::log_header_byte(m.frag_crc.at(f), n, m.get(m.frag_type, f, "frag_type"), i));
    if (!c.bytes) continue;
    for (uint64_t j = 0; j < n; ++j) {
      if (src + j >= m.base.size()) { m.bad("a source byte outside the records read", src + j); break; }
      m.st8(at + pack::lead(pack::kLog) + j, m.base[src + j]);
    }
  }
}

template <typename T>
void check_out(Model& m, Out<T>& o, const char* name) {
  for (uint64_t i = 0; i < o.v.size(); ++i) {
    const bool inside = i >= kGuard && i < kGuard + o.n;
    if (inside && o.writes[i] != 1) m.bad((std::string(name) + " element not written exactly once").c_str(), i - kGuard, o.writes[i]);
    if (!inside && (o.writes[i] || o.v[i] != T(kCanary))) m.bad((std::string(name) + " guard touched").c_str(), i);
  }
}

long run(const Call& c, const std::vector<uint8_t>& base, const Rules& rules, bool quiet) {
  Model m(c, base, quiet);
  emulate_layout(m, rules);
  emulate_fill(m);
  emulate_copy(m);
  const Want w = reference(c);
  check_out(m, m.rec_at, "rec_at"), check_out(m, m.frag_first, "frag_first"), check_out(m, m.frag_off, "frag_off");
  check_out(m, m.frag_len, "frag_len"), check_out(m, m.frag_at, "frag_at"), check_out(m, m.frag_type, "frag_type");
  check_out(m, m.frag_crc, "frag_crc");
  if (m.nfrag_writes != 1 || m.written_writes != 1) m.bad("*nfrag / *written not written exactly once");
  if (m.nfrag != w.nfrag) m.bad("*nfrag", m.nfrag, w.nfrag);
  if (m.written != w.written) m.bad("*written", m.written, w.written);
  for (uint64_t i = 0; i < c.count(); ++i)
    if (m.rec_at.at(i) != w.rec_at[i]) { m.bad("rec_at", i, m.rec_at.at(i)); break; }
  for (uint64_t i = 0; i <= c.count(); ++i)
    if (m.frag_first.at(i) != w.frag_first[i]) { m.bad("frag_first", i, m.frag_first.at(i)); break; }
  for (uint64_t f = 0; f < c.frag_cap; ++f) {
    const bool real = f < w.nfrag;
    const Phys p = real ? w.phys[f] : Phys{~uint64_t(0), 0, 0, 0};
    if (m.frag_off.at(f) != p.src || m.frag_len.at(f) != p.len || m.frag_at.at(f) != p.at || m.frag_type.at(f) != p.type ||
        m.frag_crc.at(f) != kSeed[p.type]) {
      m.bad("fragment descriptor", f, m.frag_at.at(f));
      break;
    }
  }
  if (c.bytes) {
    // the image the writer would have left in dst: fragments below frag_cap that fit, and the pads in front of records
    // whose first fragment is stored
    std::vector<uint8_t> img(c.dst_bytes + 2 * kDstGuard, 0xA5), touched(img.size(), 0);
    const auto set = [&](uint64_t at, uint8_t v) { img[kDstGuard + at] = v, touched[kDstGuard + at] = 1; };
    for (uint64_t f = 0; f < w.nfrag && f < c.frag_cap; ++f) {
      const Phys& p = w.phys[f];
      if (p.at + 7 + p.len > c.dst_bytes) continue;
      const uint32_t masked = kSeed[p.type];
      for (uint32_t i = 0; i < 4; ++i) set(p.at + i, uint8_t(masked >> (8 * i)));
      set(p.at + 4, uint8_t(p.len)), set(p.at + 5, uint8_t(p.len >> 8)), set(p.at + 6, p.type);
      for (uint64_t j = 0; j < p.len; ++j) set(p.at + 7 + j, base[p.src + j]);
    }
    for (const auto& pd : w.pads) {
      // the pad's record: the one whose first header follows it
      uint64_t rec = 0;
      while (rec < c.count() && w.rec_at[rec] != pd.first + pd.second) ++rec;
      if (rec == c.count() || w.frag_first[rec] >= c.frag_cap || pd.first + pd.second > c.dst_bytes) continue;
      for (uint64_t j = 0; j < pd.second; ++j) set(pd.first + j, 0);
    }
    for (uint64_t i = 0; i < img.size(); ++i) {
      if (m.dst[i] != img[i]) { m.bad("dst byte", i - kDstGuard, m.dst[i]); break; }
      if (m.dst_writes[i] != touched[i]) { m.bad("dst byte written other than exactly once, or not at all", i - kDstGuard, m.dst_writes[i]); break; }
      if (m.dst_writes[i] && w.written != ~uint64_t(0) && i - kDstGuard >= w.written) { m.bad("dst written at or past *written", i - kDstGuard); break; }
    }
  }
  return m.problems;
}

std::vector<uint8_t> g_base;  // the source bytes: record i of a call lies at some offset inside

void expect_ok(const Call& c) {
  ++g_cases;
  if (run(c, g_base, Rules{}, false)) ++g_failed;
}

// a call over these lengths: sources back to back from offset 3, dropped records at kSkip
Call make(const std::vector<uint64_t>& lens, uint64_t dest_length, const std::vector<uint8_t>& keep = {}, bool bytes = false,
          int cap_delta = 0, int64_t dst_delta = 0) {
  Call c;
  c.len = lens, c.keep = keep, c.dest_length = dest_length, c.bytes = bytes;
  uint64_t p = 3;
  for (uint64_t i = 0; i < lens.size(); ++i) {
    const bool k = keep.empty() || keep[i];
    c.off.push_back(k && lens[i] < kBig ? p : ~uint64_t(0));
    if (k && lens[i] < kBig) p += lens[i];
  }
  if (p > g_base.size()) {
    const uint64_t old = g_base.size();
    g_base.resize(p);
    for (uint64_t i = old; i < p; ++i) g_base[i] = uint8_t((i * 2654435761u) >> 13);
  }
  const Want w = reference(c);
  c.frag_cap = uint64_t(int64_t(w.nfrag) + cap_delta < 0 ? 0 : int64_t(w.nfrag) + cap_delta);
  c.dst_bytes = w.written == ~uint64_t(0) ? 0 : uint64_t(int64_t(w.written) + dst_delta < 0 ? 0 : int64_t(w.written) + dst_delta);
  return c;
}

std::vector<uint64_t> edge_lengths(uint32_t start) {
  const uint64_t b = start > 32761 ? 0 : start, avail = 32761 - b;
  return {0, 1, 6, 7, 8, avail ? avail - 1 : 0, avail, avail + 1, 32760, 32761, 32762, 65521, 65522, 65523, 100000};
}

int catches(const char* name, const Rules& rules, const std::vector<Call>& cases) {
  int caught = 0;
  for (const Call& c : cases)
    if (run(c, g_base, rules, true)) ++caught;
  printf("wrong rule (%s): caught in %d cases\n", name, caught);
  return caught;
}

}  // namespace

int main() {
  std::vector<Call> kept_for_rules;
  // every start offset x the edge lengths, one record a call
  for (uint32_t start = 0; start < 32768; ++start) {
    const auto lens = edge_lengths(start);
    for (size_t k = 0; k < lens.size(); ++k) {
      g_case = "start " + std::to_string(start) + " len " + std::to_string(lens[k]);
      expect_ok(make({lens[k]}, start, {}, start % 97 == 0 || start > 32750));
    }
  }
  // every sequence of up to 3 edge lengths at the edge starts
  long seq = 0;
  for (uint32_t start : {0u, 7u, 32754u, 32760u, 32761u, 32762u, 32767u}) {
    const auto L = edge_lengths(start == 32754 || start == 32760 || start == 32761 ? start : 0);
    const size_t n = L.size();
    for (size_t a = 0; a < n; ++a) {
      g_case = "seq1 at " + std::to_string(start);
      expect_ok(make({L[a]}, start, {}, true));
      for (size_t b = 0; b < n; ++b) {
        g_case = "seq2 at " + std::to_string(start) + " " + std::to_string(a) + "," + std::to_string(b);
        expect_ok(make({L[a], L[b]}, start, {}, true));
        for (size_t d = 0; d < n; ++d) {
          g_case = "seq3 at " + std::to_string(start) + " " + std::to_string(a) + "," + std::to_string(b) + "," + std::to_string(d);
          const Call c = make({L[a], L[b], L[d]}, uint64_t(start) + 32768 * (seq % 3), {}, seq % 5 == 0);
          expect_ok(c);
          if (seq % 11 == 0) kept_for_rules.push_back(c);
          ++seq;
        }
      }
    }
  }
  // random sequences: lengths around 32761 / k - 7, so that several resets fall inside one row, and rows whose first
  // and last lane leave one
  std::mt19937_64 rng(20261020);
  static const uint64_t kCounts[6] = {0, 1, 63, 64, 65, 1025};
  static const uint64_t kUnits[6] = {4673, 2333, 3269, 1631, 10913, 505};  // (unit + 7 .. 14) * k crosses 32761..32768
  for (int it = 0; it < 400; ++it) {
    const uint64_t n = it < 6 ? kCounts[it] : 1 + rng() % 300;
    const uint64_t unit = kUnits[it % 6];
    std::vector<uint64_t> lens(n);
    for (auto& l : lens) l = rng() % 7 == 0 ? rng() % 41 : unit + rng() % 8;
    std::vector<uint8_t> keep;
    if (it % 4 == 1) {  // dropped runs at both ends
      keep.assign(n, 1);
      for (uint64_t i = 0; i < n && i < uint64_t(1 + it % 5); ++i) keep[i] = 0, keep[n - 1 - i] = 0;
    } else if (it % 4 == 2) {
      keep.assign(n, 1);
      for (uint64_t i = 0; i < n; ++i) keep[i] = rng() % 3 != 0;
    } else if (it % 16 == 3) {
      keep.assign(n, 0);  // all dropped
    }
    uint64_t dest = rng() % 32768;
    g_case = "random " + std::to_string(it) + " n " + std::to_string(n);
    for (int cap_delta : {0, -1, 3}) {
      const Call c = make(lens, dest, keep, it % 3 == 0, cap_delta, it % 7 == 0 ? -1 : it % 7 == 1 ? 5 : 0);
      expect_ok(c);
      if (cap_delta == 0) kept_for_rules.push_back(c);
    }
  }
  // rows whose first and last lanes leave a reset: 7 records of 4,673..4,674 bytes fill a block to 32,761..32,768
  for (uint32_t lead = 0; lead < 8; ++lead) {
    std::vector<uint64_t> lens;
    for (uint32_t i = 0; i < lead; ++i) lens.push_back(4673);  // lane `lead - 1 + 7 k` closes a block
    for (uint32_t i = 0; i < 200; ++i) lens.push_back(i % 7 == 6 ? 4674 + i % 6 : 4673);
    g_case = "row edges lead " + std::to_string(lead);
    const Call c = make(lens, 32768 - uint64_t(lead) * 4680 % 32768, {}, true);
    expect_ok(c);
    kept_for_rules.push_back(c);
  }
  // a record of 97 fragments, alone and among others, frag_cap below, at and above
  for (int cap_delta : {0, -1, -50, 3}) {
    g_case = "97 fragments cap " + std::to_string(cap_delta);
    expect_ok(make({96 * 32761 + 5}, 0, {}, true, cap_delta));
    expect_ok(make({10, 95 * 32761 + 32751 + 1, 20, 0}, 10, {}, true, cap_delta));
  }
  // sums that saturate: a record that ends past 2^64 - 1 and every kept record behind it get kSkip and no fragment
  {
    g_case = "saturation";
    expect_ok(make({10, ~uint64_t(0) - 20, 5, 0}, 100));
    expect_ok(make({10, ~uint64_t(0), 5}, 32765));
    expect_ok(make({~uint64_t(0) - 40000, 7}, 0));
    expect_ok(make({10, ~uint64_t(0) - 20, 5}, 0, {1, 0, 1}));  // dropped: nothing saturates
    std::vector<uint64_t> many(130, 3);
    many[70] = ~uint64_t(0) - 50;  // every kept record behind it, in this row and the next two, is skipped too
    expect_ok(make(many, 5));
  }
  const int a = catches("a trailer emitted after the last record", Rules{true, false, false}, kept_for_rules);
  const int b = catches("a leftover of exactly 7 treated as a pad", Rules{false, true, false}, kept_for_rules);
  const int d = catches("a row that does not rescan behind a reset", Rules{false, false, true}, kept_for_rules);
  if (!a || !b || !d) ++g_failed;
  printf("%ld emulated calls, %ld failed\n", g_cases, g_failed);
  puts(g_failed ? "FAIL" : "PASS");
  return g_failed ? 1 : 0;
}
