// vlog_run_test.cc -- the control flow of the device value-log reader (csrc/crc32c_vlogwalk.inc: vlog_walk_kernel,
// vlog_totals_kernel) written lane by lane over a memory model, with every decision taken from csrc/vlog_run.h, the
// header the kernels themselves include -- built here with a tiny window (-DKVSEP_VLOG_WINDOW=64), so that every refill
// edge is reached in images of a few hundred bytes.  No GPU, no library.  Per emulated call:
//   * off / len / stored, *nrec and *consumed equal a plain serial walk (restated below from
//     db/value_log_reader.cc:86-108), the padding is off = len = 0 and stored = Mask(0), at cap below, at and above the
//     count and 0; ngood / good_bytes / drop_bytes equal a plain serial verdict loop (:109-122);
//   * every load is a naturally aligned 16-byte granule that holds at least one byte of [base, base + n), for a base of
//     any alignment; a step whose header is staged makes none; with n == 0 nothing is loaded;
//   * every array element in [0, cap) is written exactly once and nothing past cap (canaries); the totals read off / len
//     below min(nrec, cap) only;
//   * the step counter never exceeds n / 8.
// Three deliberately wrong rules (the payload test formed as p + 8 + l > n in 32 bits, a header read from the window
// when only part of it is staged, the store mask dropped at cap) must each be caught.  With a directory argument the
// program also runs every *.case file in it: an image and the library's host walk of it (tests/test_vlog_run_cpu.py
// writes the recorded corpus there).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DKVSEP_VLOG_WINDOW=64 -I kv-separate_amd/csrc
//       tests/cpp/vlog_run_test.cc   (one command)
#include <dirent.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "vlog_run.h"

using namespace kvsep;
namespace V = kvsep::vlogrun;

namespace {

constexpr uint64_t kPad = 3;  // canary elements on each side of every output array
constexpr uint64_t kNoBad = ~uint64_t(0);
long g_failed = 0, g_cases = 0;
std::string g_case;

struct Rules {
  bool payload_wraps = false;  // wrong: p + 8 + l > n formed in 32 bits
  bool partial_header = false; // wrong: a header is read from the window when only its first byte is staged
  bool no_store_mask = false;  // wrong: a full batch is stored without the mask by cap
};

// ---------------------------------------------------------------- the image: dense bytes, or sparse ones over a pattern
struct Image {
  uint64_t n = 0;
  bool dense = true;
  std::vector<uint8_t> b;
  std::map<uint64_t, uint8_t> sparse;
  uint8_t at(uint64_t p) const {
    if (dense) return b[p];
    auto it = sparse.find(p);
    return it != sparse.end() ? it->second : uint8_t(p * 131 + 7);
  }
  void put(uint64_t p, uint8_t v) {
    if (dense) b[p] = v;
    else sparse[p] = v;
  }
  void header(uint64_t p, uint32_t stored, uint32_t l) {
    for (int i = 0; i < 4; ++i) put(p + i, uint8_t(stored >> (8 * i))), put(p + 4 + i, uint8_t(l >> (8 * i)));
  }
};

struct Builder {  // dense images, record by record
  Image im;
  void rec(uint64_t l) {
    const uint64_t p = im.b.size();
    im.b.resize(p + 8 + l);
    im.n = im.b.size();
    im.header(p, uint32_t(0xC0DE0000u + p * 7), uint32_t(l));
    for (uint64_t i = 0; i < l; ++i) im.b[p + 8 + i] = uint8_t(0xA0 + i % 13);
  }
  void raw(std::initializer_list<uint8_t> x) { im.b.insert(im.b.end(), x), im.n = im.b.size(); }
  void junk(uint64_t k) {  // bytes that read as a length far past the end wherever a header starts among them
    im.b.insert(im.b.end(), k, 0xF1), im.n = im.b.size();
  }
};

// ---------------------------------------------------------------- the serial reference (restated, not shared code)
struct Walk {
  std::vector<uint64_t> off, len;
  std::vector<uint32_t> stored;
  uint64_t consumed = 0;
};

Walk serial_walk(const Image& im) {
  Walk w;
  uint64_t p = 0;
  while (p + 8 <= im.n) {
    uint32_t st = 0, l = 0;
    for (int i = 0; i < 4; ++i) st |= uint32_t(im.at(p + i)) << (8 * i), l |= uint32_t(im.at(p + 4 + i)) << (8 * i);
    if (l > im.n - p - 8) break;
    w.off.push_back(p + 8), w.len.push_back(l), w.stored.push_back(st);
    p += 8 + uint64_t(l);
  }
  w.consumed = p;
  return w;
}

// ---------------------------------------------------------------- the memory model
struct Model;
void bad(Model& m, const char* what, uint64_t x = 0, uint64_t y = 0);

template <typename T>
struct Out {  // an output array of cap elements between canaries
  std::vector<T> v;
  std::vector<uint8_t> w;
  uint64_t cap = 0;
  static T canary() { return T(0xC5C5C5C5C5C5C5C5ull); }
  void init(uint64_t c) { cap = c, v.assign(c + 2 * kPad, canary()), w.assign(c + 2 * kPad, 0); }
  void put(Model& m, uint64_t i, T x, const char* what) {
    if (i >= cap) { bad(m, what, i, cap); return; }
    v[kPad + i] = x;
    ++w[kPad + i];
  }
  T at(uint64_t i) const { return v[kPad + i]; }
  void check(Model& m, const char* what) const {
    for (uint64_t i = 0; i < cap; ++i)
      if (w[kPad + i] != 1) { bad(m, what, i, w[kPad + i]); break; }
    for (uint64_t i = 0; i < kPad; ++i)
      if (v[i] != canary() || v[kPad + cap + i] != canary()) bad(m, "a canary around an output array changed", i);
  }
};

struct Model {
  const Image& img;
  uint64_t addr, n, cap;  // addr = the address of image byte 0
  bool quiet;
  long problems = 0;
  Out<uint64_t> off, len;
  Out<uint32_t> stored;
  uint64_t nrec = 0, consumed = 0, ngood = 0, good_bytes = 0, drop_bytes = 0;
  int nrec_w = 0, consumed_w = 0;
  uint8_t lds[V::kWindow + V::kLdsSlack];
  bool lds_set[V::kWindow + V::kLdsSlack];
  uint64_t steps = 0, refills = 0, loads = 0;
  std::set<uint64_t> granules;

  Model(const Image& image, uint64_t a, uint64_t c, bool q) : img(image), addr(a), n(image.n), cap(c), quiet(q) {
    off.init(cap), len.init(cap), stored.init(cap);
    memset(lds, 0xDD, sizeof lds), memset(lds_set, 0, sizeof lds_set);
  }
  // one aligned 16-byte load
  void load16(uint64_t g, uint8_t out[16]) {
    ++loads;
    const bool aligned = g % V::kGranule == 0;
    const bool holds = n != 0 && g + V::kGranule > addr && g < addr + n;  // a byte of [addr, addr + n)
    if (!aligned || !holds) bad(*this, "a load outside the granules of [base, base + n)", g, addr);
    granules.insert(g);
    for (uint64_t i = 0; i < 16; ++i) {
      const uint64_t a = g + i;
      out[i] = holds && a >= addr && a - addr < n ? img.at(a - addr) : 0xEE;
    }
  }
  uint32_t lds_word(uint32_t w) {
    if (uint64_t(w) * 4 + 4 > sizeof lds) { bad(*this, "an LDS word past the window's array", w); return 0; }
    uint32_t x = 0;
    for (int i = 0; i < 4; ++i) {
      if (!lds_set[w * 4 + i]) bad(*this, "an LDS byte read before it was written", w * 4 + i);
      x |= uint32_t(lds[w * 4 + i]) << (8 * i);
    }
    return x;
  }
};

void bad(Model& m, const char* what, uint64_t x, uint64_t y) {
  if (!m.quiet && g_failed + m.problems < 20)
    printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)x, (unsigned long long)y);
  ++m.problems;
}

// ---------------------------------------------------------------- vlog_walk_kernel
struct Held {
  uint64_t off = 0, len = 0;
  uint32_t stored = 0;
};

void emit(Model& m, const Rules& rules, bool full, uint64_t first, uint32_t cnt, const Held (&my)[V::kLanes]) {
  for (uint32_t lane = 0; lane < V::kLanes; ++lane) {  // vlog_emit
    const uint64_t i = V::emit_index(first, lane);
    const bool st = rules.no_store_mask && full ? lane < cnt : V::emit_store(lane, cnt, i, m.cap);
    if (!st) continue;
    m.off.put(m, i, my[lane].off, "off[] written past cap");
    m.len.put(m, i, my[lane].len, "len[] written past cap");
    m.stored.put(m, i, my[lane].stored, "stored[] written past cap");
  }
}

void emulate_walk(Model& m, const Rules& rules) {
  for (uint32_t lane = 0; lane < V::kLanes; ++lane)
    if (lane < V::kLdsSlack / 4)
      for (int i = 0; i < 4; ++i) m.lds[V::kWindow + 4 * lane + i] = 0, m.lds_set[V::kWindow + 4 * lane + i] = true;
  const uint64_t n = m.n;
  uint64_t p = 0, k = 0, lo = 0, hi = 0;
  uint32_t sk = 0;
  Held my[V::kLanes];
  while (V::has_header(p, n)) {
    if (++m.steps > V::max_steps(n)) { bad(m, "more than n / 8 steps", m.steps, n); break; }
    const bool staged = rules.partial_header ? (p >= lo && p < hi) : V::staged(p, lo, hi);
    if (!staged) {
      ++m.refills;
      sk = V::skew(m.addr, p);
      lo = p;
      hi = V::window_hi(p, sk, n);
      const uint32_t count = V::granule_count(p, sk, hi);
      if (count == 0 || count > V::kGranules) { bad(m, "a refill of no granule or of more than the window", count); break; }
      uint8_t v[V::kLanes][V::kLoadsPerLane][16];
      for (uint32_t lane = 0; lane < V::kLanes; ++lane)  // the batch of loads, then the LDS writes
        for (uint32_t r = 0; r < V::kLoadsPerLane; ++r)
          m.load16(V::granule_addr(m.addr, p, sk, V::load_granule(V::load_slot(lane, r), count)), v[lane][r]);
      for (uint32_t lane = 0; lane < V::kLanes; ++lane)
        for (uint32_t r = 0; r < V::kLoadsPerLane; ++r) {
          const uint32_t slot = V::load_slot(lane, r);
          if (!V::slot_in_lds(slot)) continue;
          memcpy(m.lds + 16 * slot, v[lane][r], 16), memset(m.lds_set + 16 * slot, 1, 16);
        }
      if (!V::staged(p, lo, hi)) { bad(m, "the header at p is not staged by a refill at p", p, hi); break; }
    }
    const uint32_t idx = V::lds_index(p, lo, sk), w = V::lds_word(idx);
    const uint32_t w0 = m.lds_word(w), w1 = m.lds_word(w + 1), w2 = m.lds_word(w + 2);
    const uint64_t h = V::header_of_words(idx, w0, w1, w2), l = V::header_len(h);
    const bool payload = rules.payload_wraps ? !(uint32_t(uint32_t(p) + 8u + uint32_t(l)) > uint32_t(n))
                                             : V::has_payload(p, l, n);
    if (!payload) break;
    for (uint32_t lane = 0; lane < V::kLanes; ++lane)
      if (lane == V::emit_lane(k)) my[lane] = {V::rec_off(p), l, V::header_stored(h)};
    ++k;
    if (V::batch_full(k)) emit(m, rules, true, V::batch_first(k, V::kLanes), V::kLanes, my);
    p = V::next_header(p, l);
    if (p > n) { bad(m, "the position left the image", p, n); break; }
  }
  const uint32_t tail = V::tail_count(k);
  emit(m, rules, false, V::batch_first(k, tail), tail, my);
  for (uint32_t lane = 0; lane < V::kLanes; ++lane)
    for (uint64_t i = V::pad_first(k, m.cap, lane); i < m.cap; i += V::kLanes) {
      m.off.put(m, i, 0, "off[] padding past cap");
      m.len.put(m, i, 0, "len[] padding past cap");
      m.stored.put(m, i, V::kPadStored, "stored[] padding past cap");
    }
  m.nrec = k, ++m.nrec_w;
  m.consumed = p, ++m.consumed_w;
}

// ---------------------------------------------------------------- vlog_totals_kernel (lane 0)
void emulate_totals(Model& m, uint64_t first_bad) {
  const uint64_t held = V::held(m.nrec, m.cap);
  auto in = [&](const Out<uint64_t>& a, uint64_t i) -> uint64_t {
    if (i >= held) { bad(m, "the totals read off / len at or past min(nrec, cap)", i, held); return 0; }
    return a.at(i);
  };
  const uint64_t g = V::good_count(first_bad, m.nrec, m.cap);
  m.ngood = g;
  m.good_bytes = V::has_good(g) ? in(m.off, g - 1) + in(m.len, g - 1) : 0;
  m.drop_bytes = V::has_drop(g, m.nrec, m.cap) ? in(m.len, g) : 0;
}

// ---------------------------------------------------------------- one call
long run_case(const Image& img, uint64_t skew, uint64_t cap, const Rules& rules, bool quiet, const Walk* want = nullptr) {
  const Walk w = serial_walk(img);
  const uint64_t count = std::min<uint64_t>(w.off.size(), cap);
  Model m(img, 0x7f0000100000ull + skew, cap, quiet);
  emulate_walk(m, rules);
  if (want && (want->off != w.off || want->len != w.len || want->stored != w.stored || want->consumed != w.consumed))
    bad(m, "the serial walk differs from the recorded host walk");
  if (m.nrec != w.off.size()) bad(m, "nrec differs from the serial walk", m.nrec, w.off.size());
  if (m.consumed != w.consumed) bad(m, "consumed differs from the serial walk", m.consumed, w.consumed);
  if (m.nrec_w != 1 || m.consumed_w != 1) bad(m, "a result word not written exactly once");
  m.off.check(m, "an off[] element not written exactly once");
  m.len.check(m, "a len[] element not written exactly once");
  m.stored.check(m, "a stored[] element not written exactly once");
  for (uint64_t i = 0; i < cap; ++i) {
    const bool r = i < count;
    if (m.off.at(i) != (r ? w.off[i] : 0) || m.len.at(i) != (r ? w.len[i] : 0) ||
        m.stored.at(i) != (r ? w.stored[i] : V::kPadStored)) {
      bad(m, "a walk element differs from the serial walk", i);
      break;
    }
  }
  if (m.steps > V::max_steps(img.n)) bad(m, "more than n / 8 steps", m.steps);
  if (img.n == 0 && m.loads) bad(m, "an empty image was loaded from");
  // a staged step loads nothing: the loads are those of the refills, and no more refills than steps
  if (m.loads != m.refills * V::kLanes * V::kLoadsPerLane || m.refills > m.steps) bad(m, "loads outside a refill");
  // the verdicts: none bad, the first, the middle and the last record bad (padding never is)
  for (uint64_t fb : {kNoBad, uint64_t(0), count / 2, count ? count - 1 : 0}) {
    if (fb != kNoBad && fb >= count) continue;
    emulate_totals(m, fb);
    const uint64_t g = fb == kNoBad ? count : fb;
    const uint64_t gb = g ? w.off[g - 1] + w.len[g - 1] : 0, db = g < count ? w.len[g] : 0;
    if (m.ngood != g || m.good_bytes != gb || m.drop_bytes != db) bad(m, "the totals differ from the serial loop", fb);
  }
  ++g_cases;
  return m.problems;
}

// ---------------------------------------------------------------- constructed images
template <typename Visit>
void constructed(Visit visit) {  // visit(name, image, every_skew)
  const uint64_t W = V::kWindow;
  {
    Image e;
    visit("empty image", e, true);
  }
  for (uint64_t n = 1; n <= 9; ++n) {
    Builder a;
    a.junk(n);
    visit("junk of " + std::to_string(n) + " bytes", a.im, false);
    Builder z;
    z.im.b.assign(n, 0), z.im.n = n;  // n >= 8: one empty record whose stored word is 0
    visit("zeros of " + std::to_string(n) + " bytes", z.im, false);
  }
  {  // every sequence of up to three lengths from a small alphabet
    const uint64_t alpha[] = {0, 1, 7, 8, 9, 40, W - 8, W - 7, W, 100};
    for (int len = 1; len <= 3; ++len) {
      uint64_t total = 1;
      for (int i = 0; i < len; ++i) total *= 10;
      for (uint64_t code = 0; code < total; ++code) {
        Builder a;
        std::string name = "lengths";
        for (uint64_t c = code, i = 0; i < uint64_t(len); ++i, c /= 10) a.rec(alpha[c % 10]), name += " " + std::to_string(alpha[c % 10]);
        visit(name, a.im, false);
      }
    }
  }
  // the next header 9 bytes before to 1 byte after the end of the window a refill at 0 stages, for every skew of base
  for (uint64_t sk = 0; sk < 16; ++sk)
    for (uint64_t d = 0; d <= 10; ++d) {
      const uint64_t q = W - sk - 9 + d;  // where the second header starts
      if (q < 8) continue;
      Builder a;
      a.rec(q - 8), a.rec(20), a.rec(3), a.junk(5);
      visit("second header at window end " + std::to_string(int64_t(d) - 9) + " skew " + std::to_string(sk), a.im, true);
    }
  for (uint64_t t = 0; t <= 8; ++t) {  // 0 .. 8 bytes after the last record
    Builder a;
    a.rec(30), a.rec(0), a.rec(W + 5), a.junk(t);
    visit("image ending " + std::to_string(t) + " bytes after the last record", a.im, true);
  }
  for (uint64_t extra : {0, 1}) {  // l equal to the remaining bytes, and one more
    Builder a;
    a.rec(10), a.rec(50);
    const uint64_t p = a.im.b.size();
    a.rec(33);
    a.im.header(p, 0x12345678u, uint32_t(33 + extra));
    visit("a length of the remaining bytes + " + std::to_string(extra), a.im, true);
  }
  {  // a length word of 0xFFFFFFFF in a 20-byte image, alone and after a record
    Builder a;
    a.raw({1, 2, 3, 4, 0xFF, 0xFF, 0xFF, 0xFF, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9});
    visit("a length word of 0xFFFFFFFF in a 20-byte image", a.im, true);
    Builder b;
    b.rec(4);
    b.raw({1, 2, 3, 4, 0xFF, 0xFF, 0xFF, 0xFF});
    visit("a length word of 0xFFFFFFFF after a record", b.im, true);
    Builder c;  // lengths whose low bits alone look small
    c.rec(4);
    c.raw({1, 2, 3, 4, 0xF0, 0xFF, 0xFF, 0xFF, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7});
    visit("a length word of 0xFFFFFFF0", c.im, true);
  }
  for (uint64_t count : {63, 64, 65, 128, 129}) {  // the emission batches
    Builder a, b;
    for (uint64_t i = 0; i < count; ++i) a.rec(0), b.rec(i % 5);
    visit(std::to_string(count) + " empty records", a.im, true);
    visit(std::to_string(count) + " small records", b.im, false);
  }
  {  // across 4 GiB on a sparse image: only the headers are stored
    Image s;
    s.dense = false;
    const uint64_t big = (1ull << 32) - 100;
    uint64_t p = 0;
    s.header(p, 0xAAAA0001u, uint32_t(big)), p += 8 + big;  // the next header at 2^32 - 92
    s.header(p, 0xAAAA0002u, 200), p += 8 + 200;            // a record across the line
    s.header(p, 0xAAAA0003u, 0), p += 8;
    s.header(p, 0xAAAA0004u, 1000), p += 8 + 1000;
    for (uint64_t t : {0, 5, 8}) {
      s.n = p + t;
      if (t == 8) s.header(p, 0xAAAA0005u, 0xFFFFFFFFu);
      visit("n = 2^32 + " + std::to_string(s.n - (1ull << 32)), s, false);
    }
  }
}

long run_all(const Rules& rules, bool quiet) {
  long problems = 0;
  constructed([&](const std::string& name, const Image& img, bool every_skew) {
    const uint64_t c = serial_walk(img).off.size();
    for (uint64_t skew = 0; skew < 16; ++skew) {
      if (!every_skew && skew != 0 && skew != 5 && skew != 15) continue;
      for (uint64_t cap : {c ? c - 1 : 0, c, c + 3, uint64_t(0), uint64_t(64)}) {
        g_case = name + ", base skew " + std::to_string(skew) + ", cap " + std::to_string(cap);
        problems += run_case(img, skew, cap, rules, quiet) ? 1 : 0;
      }
    }
  });
  return problems;
}

// ---------------------------------------------------------------- recorded cases
// A *.case file: u64 n, u64 count, the image, then off[count] u64, len[count] u64, stored[count] u32, u64 consumed -- the
// library's host walk (kvsep_vlog_walk).
bool take(const std::vector<uint8_t>& f, size_t& at, void* dst, size_t bytes) {
  if (bytes > f.size() - at) return false;
  if (bytes) memcpy(dst, f.data() + at, bytes);
  at += bytes;
  return true;
}

long run_file(const std::string& path) {
  std::vector<uint8_t> f;
  if (FILE* fp = fopen(path.c_str(), "rb")) {
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + k);
    fclose(fp);
  }
  size_t at = 0;
  uint64_t n = 0, c = 0;
  if (!take(f, at, &n, 8) || !take(f, at, &c, 8) || n > f.size() || c > f.size()) {
    printf("FAILED %s: not a case file\n", path.c_str());
    return 1;
  }
  Image img;
  img.n = n, img.b.resize(n);
  Walk want;
  want.off.resize(c), want.len.resize(c), want.stored.resize(c);
  if (!take(f, at, img.b.data(), n) || !take(f, at, want.off.data(), c * 8) || !take(f, at, want.len.data(), c * 8) ||
      !take(f, at, want.stored.data(), c * 4) || !take(f, at, &want.consumed, 8) || at != f.size()) {
    printf("FAILED %s: truncated case file\n", path.c_str());
    return 1;
  }
  long problems = 0;
  int k = 0;
  for (uint64_t cap : {c ? c - 1 : 0, c, c + 3}) {
    g_case = path + ", cap " + std::to_string(cap);
    problems += run_case(img, uint64_t(7 * k++ + 1) % 16, cap, Rules{}, false, &want) ? 1 : 0;
  }
  return problems;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(V::kWindow == 64, "build this program with -DKVSEP_VLOG_WINDOW=64");
  if (argc > 1) {
    long files = 0;
    if (DIR* d = opendir(argv[1])) {
      std::vector<std::string> names;
      while (dirent* e = readdir(d)) {
        const std::string s = e->d_name;
        if (s.size() > 5 && s.substr(s.size() - 5) == ".case") names.push_back(s);
      }
      closedir(d);
      std::sort(names.begin(), names.end());
      for (const auto& s : names) {
        g_failed += run_file(std::string(argv[1]) + "/" + s);
        ++files;
      }
    }
    printf("%ld case files, %ld emulated calls, %ld failed\n", files, g_cases, g_failed);
    printf(g_failed || !files ? "FAIL\n" : "PASS\n");
    return g_failed || !files ? 1 : 0;
  }
  g_failed += run_all(Rules{}, false);
  printf("%ld emulated calls, %ld failed\n", g_cases, g_failed);
  const char* names[3] = {"the payload test formed as p + 8 + l > n in 32 bits",
                          "a header read from the window when only part of it is staged",
                          "the store mask dropped at cap"};
  for (int k = 0; k < 3; ++k) {
    Rules r;
    r.payload_wraps = k == 0, r.partial_header = k == 1, r.no_store_mask = k == 2;
    const long caught = run_all(r, true);
    printf("wrong rule (%s): caught in %ld cases\n", names[k], caught);
    if (!caught) ++g_failed;
  }
  printf(g_failed ? "FAIL\n" : "PASS\n");
  return g_failed ? 1 : 0;
}
