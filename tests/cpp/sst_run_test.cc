// sst_run_test.cc -- the control flow of the device SST table reader (csrc/crc32c_sstindex.inc: sst_footer_kernel,
// sst_index_count_kernel, sst_index_stop_kernel, sst_index_fill_kernel, sst_table_prep_kernel) written lane by lane over
// a memory model, with every decision taken from csrc/sst_run.h, the header the kernels themselves include.  No GPU, no
// library.  The prep kernel is run as the table form runs it -- one slot on the index block alone before the walk, cap
// slots after it, with the status and count words the other kernels left -- and its rule on a table of handles at the
// image's edge besides.  Per emulated call:
//   * off / len / *nblocks / *status equal a plain serial walk of the block (restated below from table/block.cc and
//     BlockHandle::DecodeFrom, not shared code), at cap below, at and above the count; on a block with no error they
//     also equal Block::Iter's loop, which never looks at the restart array; the footer equals Footer::DecodeFrom
//     restated;
//   * every output element is written exactly once for exactly cap elements, the canaries around them stay;
//   * every image byte read lies inside the index block (its type byte in the table form) or the footer;
//   * no scratch word is read that the call did not write, none is written past the runs the scratch holds.
// The offsets pass between stop and fill is taken by its contract (an exclusive prefix sum over the runs before
// *keep_before, kSkip from there on, and the total): it has a model of its own, offsets_run_test.cc.  Three
// deliberately wrong rules (a run allowed to end past its end offset, shared unchecked on a run's first entry, the stop
// taken from the highest run with an error) must each be caught.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kv-separate_amd/csrc tests/cpp/sst_run_test.cc
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sst_run.h"

using namespace kvsep;
namespace S = kvsep::sst;
typedef std::vector<uint8_t> Bytes;

namespace {

constexpr uint64_t kPad = 3;  // canary elements on each side of every output array
constexpr uint64_t kCanary = 0xC5C5C5C5C5C5C5C5ull;
long g_failed = 0, g_cases = 0;
std::string g_case;

// ---------------------------------------------------------------- the wrong rules
struct EndsPastRun : S::Rule {  // wrong: an entry may run to the end of the block's entries, past its run's end
  static bool fits(uint64_t need, uint64_t p, uint64_t, uint64_t restart_offset) { return need <= restart_offset - p; }
};
struct FirstSharedAny : S::Rule {  // wrong: shared is not checked on a run's first entry
  static bool first_shared_ok(uint32_t) { return true; }
};
struct StopHighest : S::Rule {  // wrong: the highest run with an error stops the walk
  static uint64_t stop_pick(uint64_t a, uint64_t b) {
    if (a == S::kNone) return b;
    if (b == S::kNone) return a;
    return a > b ? a : b;
  }
};

// ---------------------------------------------------------------- the serial reference (restated, not shared code)
struct Ref {
  std::vector<uint64_t> off, len;
  uint32_t status = 0;
};

uint32_t ref_le32(const Bytes& b, uint64_t p) {
  return uint32_t(b[p]) | uint32_t(b[p + 1]) << 8 | uint32_t(b[p + 2]) << 16 | uint32_t(b[p + 3]) << 24;
}

// util/coding.cc GetVarint64Ptr / GetVarint32Ptr: at most `maxbytes` bytes, none at or past limit
bool ref_varint(const Bytes& b, uint64_t& p, uint64_t limit, int maxbytes, uint64_t& v) {
  v = 0;
  for (int i = 0; i < maxbytes && p < limit; ++i) {
    const uint64_t byte = b[p++];
    v |= (byte & 127) << (7 * i);
    if (byte < 128) {
      if (maxbytes == 5) v &= 0xffffffffull;
      return true;
    }
  }
  return false;
}

Ref ref_walk(const Bytes& b) {
  Ref r;
  const uint64_t n = b.size();
  r.status = 4;
  if (n < 4) return r;
  const uint64_t nr = ref_le32(b, n - 4);
  if (nr > (n - 4) / 4) return r;
  const uint64_t ro = n - 4 * (1 + nr);
  for (uint64_t k = 0; k < nr; ++k) {
    const uint64_t s = ref_le32(b, ro + 4 * k);
    r.status = 4;
    if (k == 0 ? s != 0 : (s <= ref_le32(b, ro + 4 * (k - 1)) || s >= ro)) return r;
    uint64_t e = ro;
    if (k + 1 < nr) {
      const uint64_t nx = ref_le32(b, ro + 4 * (k + 1));
      if (nx > s && nx < ro) e = nx;
    }
    uint64_t p = s, prev_key = 0;
    bool first = true;
    while (p < e) {
      uint64_t shared, non_shared, vlen, o, l;
      r.status = 5;
      if (e - p < 3) return r;
      if (!ref_varint(b, p, e, 5, shared) || !ref_varint(b, p, e, 5, non_shared) || !ref_varint(b, p, e, 5, vlen))
        return r;
      if (first ? shared != 0 : shared > prev_key) return r;
      if (non_shared + vlen > e - p) return r;
      uint64_t v = p + non_shared;
      const uint64_t vend = v + vlen;
      r.status = 6;
      if (!ref_varint(b, v, vend, 10, o) || !ref_varint(b, v, vend, 10, l)) return r;
      r.off.push_back(o), r.len.push_back(l);
      p = vend;
      prev_key = shared + non_shared;
      first = false;
    }
  }
  r.status = 0;
  return r;
}

// Block::Iter from SeekToFirst to the end (table/block.cc): entries from 0 to restart_offset, key_ carried along; the
// restart array is not looked at.  false: the iterator reports corruption.
bool ref_iter(const Bytes& b, Ref* out) {
  const uint64_t n = b.size();
  if (n < 4) return false;
  const uint64_t nr = ref_le32(b, n - 4);
  if (nr > (n - 4) / 4) return false;
  if (nr == 0) return true;
  const uint64_t ro = n - 4 * (1 + nr);
  uint64_t p = 0, key = 0;
  while (p < ro) {
    uint64_t shared, non_shared, vlen, o, l;
    if (ro - p < 3) return false;
    if (!ref_varint(b, p, ro, 5, shared) || !ref_varint(b, p, ro, 5, non_shared) || !ref_varint(b, p, ro, 5, vlen))
      return false;
    if (non_shared + vlen > ro - p || key < shared) return false;
    uint64_t v = p + non_shared;
    if (!ref_varint(b, v, v + vlen, 10, o) || !ref_varint(b, v, p + non_shared + vlen, 10, l)) return false;
    out->off.push_back(o), out->len.push_back(l);
    p += non_shared + vlen;
    key = shared + non_shared;
  }
  return true;
}

struct RefFooter {
  uint64_t h[4] = {0, 0, 0, 0};
  uint32_t status = 1;
};
bool ref_usable(uint64_t off, uint64_t len, uint64_t n) {
  const unsigned __int128 end = (unsigned __int128)off + len + 5;
  return end <= n;
}
RefFooter ref_footer(const Bytes& b) {
  RefFooter f;
  const uint64_t n = b.size();
  if (n < 48) return f;
  uint64_t magic = 0;
  for (int i = 7; i >= 0; --i) magic = magic << 8 | b[n - 8 + i];
  if (magic != 0xdb4775248b80fb57ull) return f;
  uint64_t p = n - 48, h[4];
  for (int k = 0; k < 4; ++k)
    if (!ref_varint(b, p, n - 8, 10, h[k])) return f;
  if (!ref_usable(h[0], h[1], n) || !ref_usable(h[2], h[3], n)) return f;
  memcpy(f.h, h, sizeof h);
  f.status = 0;
  return f;
}

// ---------------------------------------------------------------- the memory model
struct Model;
void bad(Model& m, const char* what, uint64_t x = 0, uint64_t y = 0);

struct Word {
  uint64_t v = 0;
  bool set = false;
};

struct Out {  // an output array of cap elements between canaries
  std::vector<uint64_t> v;
  std::vector<uint8_t> w;
  uint64_t cap = 0;
  void init(uint64_t c) { cap = c, v.assign(c + 2 * kPad, kCanary), w.assign(c + 2 * kPad, 0); }
  void put(Model& m, uint64_t i, uint64_t x, const char* what) {
    if (i >= cap) { bad(m, what, i, cap); return; }
    v[kPad + i] = x;
    ++w[kPad + i];
  }
  uint64_t at(uint64_t i) const { return v[kPad + i]; }
  void check(Model& m, const char* what) const {
    for (uint64_t i = 0; i < cap; ++i)
      if (w[kPad + i] != 1) { bad(m, what, i, w[kPad + i]); break; }
    for (uint64_t i = 0; i < kPad; ++i)
      if (v[i] != kCanary || v[kPad + cap + i] != kCanary) bad(m, "a canary around an output array changed", i);
  }
};

struct Model {
  const Bytes& img;
  uint64_t n, cap, runs;
  bool quiet;
  long problems = 0;
  std::vector<uint8_t> touched;
  Out off, len;
  Word nblocks, status, stop[2];
  int status_w = 0;
  std::vector<Word> cnt, errbase, wgstop;
  Model(const Bytes& image, uint64_t c, uint64_t r, bool q) : img(image), n(image.size()), cap(c), runs(r), quiet(q) {
    touched.assign(n, 0);
    off.init(cap), len.init(cap);
    cnt.resize(runs), errbase.resize(runs), wgstop.resize(S::grid_for(runs));
  }
  uint64_t rd(std::vector<Word>& a, uint64_t i, const char* what) {
    if (i >= a.size()) { bad(*this, what, i); return 0; }
    if (!a[i].set) bad(*this, "a scratch word read before this call wrote it", i);
    return a[i].v;
  }
  uint64_t rd(const Word& w) {
    if (!w.set) bad(*this, "a word read before this call wrote it");
    return w.v;
  }
  void wr(std::vector<Word>& a, uint64_t i, uint64_t v, const char* what) {
    if (i >= a.size()) { bad(*this, what, i); return; }
    a[i] = {v, true};
  }
};

void bad(Model& m, const char* what, uint64_t x, uint64_t y) {
  if (!m.quiet && g_failed + m.problems < 20)
    printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)x, (unsigned long long)y);
  ++m.problems;
}

struct Mem {  // rd(p): byte p of the image, recorded
  Model* m;
  uint8_t operator()(uint64_t p) const {
    if (p >= m->n) { bad(*m, "an image byte outside [0, n) was read", p, m->n); return 0; }
    m->touched[p] = 1;
    return m->img[p];
  }
};

// ---------------------------------------------------------------- the kernels, lane by lane
struct Table {  // the table form's extra inputs
  uint64_t handles[4];
  uint32_t footer_status, crc, stored;  // the index block's checksum as computed and as stored (masked)
};

// sst_footer_kernel
S::Footer emulate_footer(Model& m) {
  Mem rd{&m};
  S::Footer out{{0, 0, 0, 0}, 99};
  for (uint32_t t = 0; t < S::kFooterThreads; ++t)
    if (t == 0) out = S::footer(rd, m.n);
  return out;
}

template <class R>
void emulate_walk(Model& m, uint64_t ioff, uint64_t ilen, const Table* tab) {
  Mem rd{&m};
  const bool table = tab != nullptr;
  // sst_stop_reduce: the tree in LDS
  const auto reduce = [](std::vector<uint64_t>& sh) {
    for (uint32_t d = S::kThreads / 2; d; d >>= 1)
      for (uint32_t t = 0; t < d; ++t) sh[t] = R::stop_pick(sh[t], sh[t + d]);
    return sh[0];
  };
  const uint64_t nwg = S::grid_for(m.runs);
  for (uint64_t wg = 0; wg < nwg; ++wg) {  // sst_index_count_kernel
    std::vector<uint64_t> sh(S::kThreads);
    for (uint32_t t = 0; t < S::kThreads; ++t) {
      const uint64_t r = wg * S::kThreads + t;
      sh[t] = S::kNone;
      if (r >= m.runs) continue;
      uint32_t pre = S::kOk;
      if (table) {
        const uint32_t fs = tab->footer_status;
        pre = S::gate(fs, fs ? 0 : tab->crc, fs ? 0 : S::unmask(tab->stored), fs ? uint8_t(0) : rd(ioff + ilen));
      }
      const S::Counted c = S::count_lane<R>(rd, m.n, ioff, ilen, pre, m.runs, r);
      m.wr(m.cnt, r, c.cnt, "cnt[] written past the runs the scratch holds");
      m.wr(m.errbase, r, c.err, "err[] written past the runs the scratch holds");
      sh[t] = S::stop_candidate(r, c.err);
    }
    m.wr(m.wgstop, wg, reduce(sh), "wgstop[] written past the count kernel's workgroups");
  }
  {  // sst_index_stop_kernel: one workgroup, strided over the workgroups' words, then the tree
    std::vector<uint64_t> sh(S::kThreads);
    for (uint32_t t = 0; t < S::kThreads; ++t) {
      uint64_t v = S::kNone;
      for (uint64_t w = t; w < nwg; w += S::kThreads) v = R::stop_pick(v, m.rd(m.wgstop, w, "wgstop[]"));
      sh[t] = v;
    }
    const uint64_t s = reduce(sh), e = s == S::kNone ? 0 : m.rd(m.errbase, s, "err[stop]");
    m.stop[0] = {S::keep_before(s, e), true};
    m.stop[1] = {e, true};
  }
  {  // the offsets pass over cnt[], by its contract; base[] goes over err[]
    const uint64_t before = m.rd(m.stop[0]);
    uint64_t acc = 0;
    for (uint64_t r = 0; r < m.runs; ++r) {
      const uint64_t c = m.rd(m.cnt, r, "cnt[]");
      m.wr(m.errbase, r, r < before ? acc : S::kSkip, "base[]");
      if (r < before) acc += c;
    }
    m.nblocks = {acc, true};
  }
  const uint64_t limit = S::data_cap(table, m.cap);
  const uint64_t lanes = S::pad_grid(m.runs, m.cap) * S::kThreads;  // sst_index_fill_kernel
  for (uint64_t g = 0; g < lanes; ++g) {
    if (g < m.runs) {
      const uint64_t b = m.rd(m.errbase, g, "base[]");
      S::fill_lane<R>(rd, ioff, ilen, g, b, limit, [&](uint64_t k, uint64_t o, uint64_t l) {
        const uint64_t i = b + k;
        if (i >= limit) return false;
        m.off.put(m, i, o, "off[] written past the room for data blocks");
        m.len.put(m, i, l, "len[] written past the room for data blocks");
        return true;
      });
    }
    const uint64_t nblocks = m.rd(m.nblocks), mm = S::held(nblocks, limit);
    for (uint64_t i = mm + g; i < m.cap; i += lanes) {
      m.off.put(m, i, S::after_data(table, i, mm, table ? tab->handles : nullptr, 0), "off[] padding past cap");
      m.len.put(m, i, S::after_data(table, i, mm, table ? tab->handles : nullptr, 1), "len[] padding past cap");
    }
    if (g == 0) {
      m.status = {S::final_status(S::code_of(m.rd(m.stop[1])), table, nblocks, m.cap), true};
      ++m.status_w;
    }
  }
}

// ---------------------------------------------------------------- one emulated call against the reference
// The image: `lead` bytes, the block, 5 trailer bytes (type byte first), `trail` bytes.
struct Image {
  Bytes img;
  uint64_t ioff, ilen;
};
Image place(const Bytes& blk, uint64_t lead = 7, uint64_t trail = 9, uint8_t type = 0) {
  Image im;
  im.img.assign(lead, 0xAB);
  im.img.insert(im.img.end(), blk.begin(), blk.end());
  im.img.push_back(type);
  for (int i = 0; i < 4; ++i) im.img.push_back(0xCD);
  im.img.insert(im.img.end(), trail, 0xEF);
  im.ioff = lead, im.ilen = blk.size();
  return im;
}

// Expected outputs of the walk alone from the serial reference.
struct Expect {
  std::vector<uint64_t> off, len;  // cap elements
  uint64_t nblocks;
  uint32_t status;
};
Expect expect_walk(const Ref& r, uint64_t cap) {
  Expect e;
  e.off.assign(cap, 0), e.len.assign(cap, 0);
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, r.off.size()); ++i) e.off[i] = r.off[i], e.len[i] = r.len[i];
  e.nblocks = r.off.size();
  e.status = r.status;
  return e;
}
// ... and of the table form: data slots, the footer's two handles, padding.
Expect expect_table(const Ref& r, uint32_t pre, const uint64_t h[4], uint64_t cap) {
  Expect e;
  e.off.assign(cap, 0), e.len.assign(cap, 0);
  const uint64_t cnt = pre ? 0 : r.off.size(), m = std::min<uint64_t>(cnt, cap - 2);
  for (uint64_t i = 0; i < m; ++i) e.off[i] = r.off[i], e.len[i] = r.len[i];
  e.off[m] = h[0], e.len[m] = h[1], e.off[m + 1] = h[2], e.len[m + 1] = h[3];
  e.nblocks = cnt;
  e.status = pre ? pre : r.status ? r.status : cnt + 2 > cap ? 7 : 0;
  return e;
}

template <class R>
long run_call(const Image& im, uint64_t cap, uint64_t runs, const Table* tab, const Expect& want, bool quiet) {
  Model m(im.img, cap, runs, quiet);
  emulate_walk<R>(m, im.ioff, im.ilen, tab);
  m.off.check(m, "an off[] element not written exactly once");
  m.len.check(m, "a len[] element not written exactly once");
  if (m.status_w != 1) bad(m, "*status not written exactly once", m.status_w);
  if (m.rd(m.nblocks) != want.nblocks) bad(m, "*nblocks differs from the serial walk", m.nblocks.v, want.nblocks);
  if (m.rd(m.status) != want.status) bad(m, "*status differs from the serial walk", m.status.v, want.status);
  for (uint64_t i = 0; i < cap; ++i)
    if (m.off.at(i) != want.off[i] || m.len.at(i) != want.len[i]) {
      bad(m, "off[] / len[] differ from the serial walk", i, m.off.at(i));
      break;
    }
  const uint64_t hi = im.ioff + im.ilen + (tab ? 1 : 0);  // the table form reads the type byte
  for (uint64_t p = 0; p < m.n; ++p)
    if (m.touched[p] && (p < im.ioff || p >= hi)) {
      bad(m, "an image byte outside the index block was read", p);
      break;
    }
  ++g_cases;
  return m.problems;
}

struct Wrong {
  const char* name;
  long caught = 0;
};
Wrong g_wrong[3] = {{"a run allowed to end past its end offset"},
                    {"shared unchecked on a run's first entry"},
                    {"the stop taken from the highest run with an error"}};

// One block at one cap: the sound rules must agree with the reference, and each wrong rule is given its chance.
void check_block(const Bytes& blk, uint64_t cap, uint64_t runs, bool wrongs) {
  const Ref ref = ref_walk(blk);
  if (ref.status == 0) {
    Ref it;
    if (!ref_iter(blk, &it) || it.off != ref.off || it.len != ref.len) {
      printf("FAILED %s: the serial walk differs from Block::Iter's loop on a block with no error\n", g_case.c_str());
      ++g_failed;
    }
  }
  const Image im = place(blk);
  const bool over = blk.size() >= 4 && ref_le32(blk, blk.size() - 4) > runs;
  Ref eff = ref;
  if (over) eff = Ref{{}, {}, 4};  // more runs than the scratch holds: stopped before any run
  const Expect want = expect_walk(eff, cap);
  g_failed += run_call<S::Rule>(im, cap, runs, nullptr, want, false);
  if (!wrongs) return;
  if (run_call<EndsPastRun>(im, cap, runs, nullptr, want, true)) ++g_wrong[0].caught;
  if (run_call<FirstSharedAny>(im, cap, runs, nullptr, want, true)) ++g_wrong[1].caught;
  if (run_call<StopHighest>(im, cap, runs, nullptr, want, true)) ++g_wrong[2].caught;
}

void check_caps(const Bytes& blk, bool wrongs) {
  const Ref ref = ref_walk(blk);
  const uint64_t cnt = ref.off.size();
  const uint64_t nr = blk.size() >= 4 ? std::min<uint64_t>(ref_le32(blk, blk.size() - 4), blk.size() / 4) : 0;
  const uint64_t runs = std::max<uint64_t>(nr, 1) + 2;
  if (cnt) check_block(blk, cnt - 1, runs, wrongs);
  check_block(blk, cnt, runs, wrongs);
  check_block(blk, cnt + 3, runs, wrongs);
}

// ---------------------------------------------------------------- block builders
void put_varint(Bytes& b, uint64_t v, int width = 0) {  // width > 0: padded to that many bytes (a valid, longer form)
  int k = 0;
  while (v >= 128 || k + 1 < width) {
    b.push_back(uint8_t(v & 127) | 128);
    v >>= 7;
    ++k;
  }
  b.push_back(uint8_t(v));
}
void put_le32(Bytes& b, uint32_t v) {
  for (int i = 0; i < 4; ++i) b.push_back(uint8_t(v >> (8 * i)));
}

struct Kind {
  uint32_t shared, key;  // key = non_shared bytes
  uint64_t off, len;     // the handle: their values pick the varint widths (1, 2, 5, 9, 10 bytes)
  int field_width;       // of the three entry fields: 1, or 2 (the slow path of DecodeEntry)
  int cut;               // bytes taken off the value: > 0 makes it too short for its handle
  int extra;             // bytes after the handle inside the value: ignored
};
const Kind kKinds[8] = {
    {0, 2, 5, 7, 1, 0, 0},                           // 1-byte fields everywhere
    {1, 1, 300, 1ull << 28, 1, 0, 0},                // shared 1 (illegal at a restart point); 2- and 5-byte varints
    {0, 3, 1ull << 56, (1ull << 63) + 1, 1, 0, 0},   // 9- and 10-byte varints
    {0, 1, 9, 11, 2, 0, 0},                          // 2-byte entry fields
    {9, 1, 13, 15, 1, 0, 0},                         // shared above any previous key here
    {0, 2, 200, 17, 1, 1, 0},                        // the value too short
    {0, 0, 400, 500, 1, 0, 3},                       // an empty key delta, bytes after the handle
    {2, 2, 21, 23, 2, 0, 0},                         // shared 2 with 2-byte fields
};

Bytes build(const std::vector<int>& kinds, uint32_t interval) {
  Bytes b;
  std::vector<uint32_t> restarts;
  for (size_t j = 0; j < kinds.size(); ++j) {
    const Kind& k = kKinds[kinds[j]];
    if (j % interval == 0) restarts.push_back(uint32_t(b.size()));
    Bytes value;
    put_varint(value, k.off);
    put_varint(value, k.len);
    for (int i = 0; i < k.cut && !value.empty(); ++i) value.pop_back();
    value.insert(value.end(), size_t(k.extra), 0x5A);
    put_varint(b, k.shared, k.field_width);
    put_varint(b, k.key, k.field_width);
    put_varint(b, value.size(), k.field_width);
    b.insert(b.end(), k.key, 0x6B);
    b.insert(b.end(), value.begin(), value.end());
  }
  if (restarts.empty()) restarts.push_back(0);  // BlockBuilder starts with one restart point
  for (uint32_t r : restarts) put_le32(b, r);
  put_le32(b, uint32_t(restarts.size()));
  return b;
}

void small_blocks() {
  for (uint32_t interval = 1; interval <= 3; ++interval)
    for (int n = 0; n <= 4; ++n) {
      std::vector<int> kinds(n, 0);
      for (;;) {
        char name[96];
        snprintf(name, sizeof name, "interval %u kinds", interval);
        g_case = name;
        for (int k : kinds) g_case += " " + std::to_string(k);
        check_caps(build(kinds, interval), true);
        int i = 0;
        while (i < n && ++kinds[i] == 8) kinds[i++] = 0;
        if (i == n) break;
      }
    }
}

void tail_mutations() {
  const std::vector<int> picks[3] = {{0, 6, 2, 3}, {0, 1, 0, 7}, {2, 0, 3, 1}};
  for (int w = 0; w < 3; ++w) {
    const Bytes base = build(picks[w], w + 1);
    const uint64_t nr = ref_le32(base, base.size() - 4), tail = 4 * (1 + nr);
    for (uint64_t at = base.size() - tail; at < base.size(); ++at)
      for (int v = 0; v < 256; ++v) {
        if (v == base[at]) continue;
        Bytes b = base;
        b[at] = uint8_t(v);
        g_case = "tail mutation of block " + std::to_string(w) + " byte " + std::to_string(at) + " = " +
                 std::to_string(v);
        // a mutated count can promise up to len / 4 runs: the scratch holds them all here
        check_block(b, 6, b.size() / 4 + 1, true);
      }
  }
}

void restart_counts() {
  for (uint64_t nr : {0ull, 1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull}) {
    Bytes b;
    if (nr == 0) {
      put_le32(b, 0);  // no restart at all: an empty, valid block
    } else {
      std::vector<int> kinds(nr);
      for (uint64_t j = 0; j < nr; ++j) kinds[j] = (j % 3 == 0) ? 0 : (j % 3 == 1 ? 2 : 3);
      b = build(kinds, 1);
    }
    g_case = "restart count " + std::to_string(nr);
    check_caps(b, false);
    if (nr >= 64) {  // an error in a late run and one in an early run: the early one wins
      Bytes c = b;
      const uint64_t ro = c.size() - 4 * (1 + nr);
      c[ref_le32(c, ro + 4 * (nr - 2))] = 1;  // shared = 1 on the first entry of run nr - 2
      c[ref_le32(c, ro + 4 * 5) + 2] = 0;     // value_len = 0 in run 5: no handle
      g_case += " with two errors";
      check_caps(c, true);
    }
    if (nr >= 2) {  // a run count over what the scratch holds: stopped with BAD_RESTARTS, nothing written past it
      g_case = "restart count " + std::to_string(nr) + " over the reservation";
      check_block(b, nr, nr - 1, false);
      check_block(b, 3, 1, false);
    }
  }
}

// ---------------------------------------------------------------- the footer, the table form, the read check's prep
Bytes footer_bytes(const uint64_t h[4], const int width[4]) {
  Bytes f;
  for (int k = 0; k < 4; ++k) put_varint(f, h[k], width[k]);
  f.resize(40, 0);
  for (int i = 0; i < 8; ++i) f.push_back(uint8_t(0xdb4775248b80fb57ull >> (8 * i)));
  return f;
}

void check_footer(const Bytes& img) {
  Model m(img, 0, 1, false);
  const S::Footer got = emulate_footer(m);
  const RefFooter want = ref_footer(img);
  if (got.status != want.status || memcmp(got.h, want.h, sizeof want.h)) bad(m, "the footer differs", got.status);
  for (uint64_t p = 0; p + 48 < m.n; ++p)
    if (m.touched[p]) { bad(m, "a byte before the footer was read", p); break; }
  g_failed += m.problems;
  ++g_cases;
}

void footers() {
  const int w1[4] = {0, 0, 0, 0}, w10[4] = {10, 9, 5, 2};
  for (uint64_t n : {48ull, 49ull, 200ull}) {
    // handles at off + len + 5 = n, at n + 1, and with sums past 2^64
    const uint64_t hs[][4] = {{0, n - 5, 0, n - 5}, {0, n - 4, 0, 0}, {0, 0, 1, n - 5}, {n - 5, 0, n, 0},
                              {~0ull - 2, 10, 0, 0}, {0, 0, 10, ~0ull - 2}, {~0ull, ~0ull, 0, 0}, {3, 4, 5, 6}};
    for (const auto& h : hs)
      for (const int* w : {w1, w10}) {
        Bytes f = footer_bytes(h, w);
        if (f.size() != 48) continue;  // the four varints did not fit: not a footer this builder can make
        Bytes img(n - 48, 0x11);
        img.insert(img.end(), f.begin(), f.end());
        g_case = "footer n " + std::to_string(n) + " handle " + std::to_string(h[0]) + "," + std::to_string(h[1]);
        check_footer(img);
        Bytes wrong = img;
        wrong[n - 3] ^= 0x40;  // a wrong magic
        check_footer(wrong);
      }
  }
  g_case = "footer shorter than 48";
  check_footer(Bytes(47, 0x80));
  check_footer(Bytes(0));
  g_case = "footer varint leaves the 40 bytes";
  const uint64_t z[4] = {0, 0, 0, 0};
  Bytes f = footer_bytes(z, w1);
  for (int i = 0; i < 40; ++i) f[i] = 0x80;
  check_footer(f);
  for (int i = 3; i < 40; ++i) f[i] = 0x81;  // three good ones, then one that never ends
  f[0] = f[1] = f[2] = 0;
  check_footer(f);
}

// sst_table_prep_kernel, lane by lane: count slots of off / len; nblocks == nullptr is the one-slot call on the index
// block alone, made while *status still holds the footer kernel's word.
void emulate_prep(Model& m, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, uint64_t count,
                  const uint64_t* nblocks, uint32_t status, uint64_t cap, std::vector<Word>& len1,
                  std::vector<Word>& stored) {
  Mem rd{&m};
  for (uint64_t i = 0; i < S::grid_for(count) * S::kThreads; ++i) {
    if (i >= count) continue;
    const uint64_t real = nblocks ? S::listed(status, *nblocks, cap) : (status == S::kBadFooter ? 0 : 1);
    const uint64_t o = off[i], l = len[i];
    const S::Prep p = S::prep(i < real, o, l, m.n);
    const uint32_t st = p.read ? S::le32(rd, o + l + 1) : p.stored;
    m.wr(len1, i, p.len1, "len1[] written past its slots");
    m.wr(stored, i, st, "stored[] written past its slots");
  }
}

// The table form's two prep calls around the walk, against the slot rules restated: a listed slot with a usable handle
// gets len + 1 and the image's stored word, a listed one that leaves the image 0 and a word that cannot match,
// padding 0 and Mask(0); the image is read only inside the index block, its type byte and those stored words.
void check_prep(const Image& im, uint64_t cap, const Table& tab, const char* what) {
  g_case = std::string("prep, ") + what + ", cap " + std::to_string(cap);
  Model m(im.img, cap, 9, false);
  std::vector<Word> len1(cap), stored(cap);
  const std::vector<uint64_t> ioff{tab.handles[2]}, ilen{tab.handles[3]};
  emulate_prep(m, ioff, ilen, 1, nullptr, tab.footer_status, cap, len1, stored);
  const bool foot_ok = tab.footer_status == 0;
  if (len1[0].v != (foot_ok ? ilen[0] + 1 : 0)) bad(m, "the index block's own slot", len1[0].v);
  emulate_walk<S::Rule>(m, tab.handles[2], tab.handles[3], &tab);
  std::vector<uint64_t> off(cap), len(cap);
  for (uint64_t i = 0; i < cap; ++i) off[i] = m.off.at(i), len[i] = m.len.at(i);
  const uint64_t nblocks = m.rd(m.nblocks);
  for (auto& w : len1) w.set = false;
  for (auto& w : stored) w.set = false;
  emulate_prep(m, off, len, cap, &nblocks, uint32_t(m.rd(m.status)), cap, len1, stored);
  const uint64_t listed = foot_ok ? std::min<uint64_t>(nblocks, cap - 2) + 2 : 0;
  std::vector<uint8_t> allowed(m.n, 0);
  if (foot_ok) {
    for (uint64_t p = im.ioff; p < im.ioff + im.ilen + 5; ++p) allowed[p] = 1;  // the block, its type byte and word
  }
  for (uint64_t i = 0; i < cap; ++i) {
    uint64_t want1 = 0;
    uint32_t wants = 0xa282ead8u;  // Mask(0)
    if (i < listed) {
      if (ref_usable(off[i], len[i], m.n)) {
        want1 = len[i] + 1;
        wants = ref_le32(im.img, off[i] + len[i] + 1);
        for (int k = 1; k < 5; ++k) allowed[off[i] + len[i] + k] = 1;
      } else {
        wants = ~0xa282ead8u;
      }
    }
    if (!len1[i].set || !stored[i].set) bad(m, "a slot of the SST arrays not written", i);
    if (len1[i].v != want1 || uint32_t(stored[i].v) != wants) bad(m, "len1[] / stored[] differ", i, len1[i].v);
  }
  for (uint64_t p = 0; p < m.n; ++p)
    if (m.touched[p] && !allowed[p]) { bad(m, "prep: an image byte outside the listed blocks' words was read", p); break; }
  g_failed += m.problems;
  ++g_cases;
}

void table_form() {
  const Bytes blk = build({0, 6, 2, 3, 0}, 1);
  const Ref ref = ref_walk(blk);
  const Image im = place(blk, 11, 60);
  Table t{{3, 4, im.ioff, im.ilen}, 0, 0x12345678u, 0};
  t.stored = (((t.crc >> 15) | (t.crc << 17)) + 0xa282ead8u);  // Mask(crc)
  for (uint64_t cap : {2ull, 3ull, 6ull, 7ull, 8ull, 12ull}) {
    g_case = "table form cap " + std::to_string(cap);
    g_failed += run_call<S::Rule>(im, cap, 9, &t, expect_table(ref, 0, t.handles, cap), false);
    Table badsum = t;
    badsum.stored ^= 0x100;
    g_case = "table form, index checksum, cap " + std::to_string(cap);
    g_failed += run_call<S::Rule>(im, cap, 9, &badsum, expect_table(ref, 2, t.handles, cap), false);
    Table nofoot{{0, 0, 0, 0}, 1, 0, 0};
    check_prep(im, cap, t, "table form");
    check_prep(im, cap, badsum, "index checksum");
    check_prep(im, cap, nofoot, "bad footer");
    g_case = "table form, bad footer, cap " + std::to_string(cap);
    {
      Image at0 = im;
      at0.ioff = 0, at0.ilen = 0;  // what the footer kernel leaves in handles[2..4)
      Model m(at0.img, cap, 9, false);
      emulate_walk<S::Rule>(m, 0, 0, &nofoot);
      const Expect want = expect_table(ref, 1, nofoot.handles, cap);
      if (m.rd(m.status) != 1 || m.rd(m.nblocks) != 0) bad(m, "a bad footer must list nothing", m.status.v);
      for (uint64_t i = 0; i < cap; ++i)
        if (m.off.at(i) != want.off[i] || m.len.at(i) != want.len[i]) bad(m, "a bad footer must list nothing", i);
      for (uint64_t p = 0; p < m.n; ++p)
        if (m.touched[p]) { bad(m, "a bad footer: an image byte was read", p); break; }
      g_failed += m.problems;
      ++g_cases;
    }
  }
  const Image comp = place(blk, 11, 60, 1);  // a type byte of 1: compressed, with a good checksum
  g_case = "table form, compressed index";
  g_failed += run_call<S::Rule>(comp, 8, 9, &t, expect_table(ref, 3, t.handles, 8), false);
  Table both = t;
  both.stored ^= 1;
  g_case = "table form, compressed index with a bad checksum: the checksum comes first";
  g_failed += run_call<S::Rule>(comp, 8, 9, &both, expect_table(ref, 2, t.handles, 8), false);
  if (S::unmask(t.stored) != t.crc || S::kMaskOfZero != 0xa282ead8u) {
    printf("FAILED unmask is not Mask's inverse\n");
    ++g_failed;
  }
}

void prep_rules() {
  const uint64_t n = 1000;
  struct { bool real; uint64_t off, len; uint64_t len1; bool read; uint32_t stored; } cases[] = {
      {true, 0, n - 5, n - 4, true, 0},                       // off + len + 5 = n
      {true, 0, n - 4, 0, false, S::kNoMatch},                // ... = n + 1
      {true, n - 5, 0, 1, true, 0},
      {true, n - 4, 0, 0, false, S::kNoMatch},
      {true, ~0ull - 2, 10, 0, false, S::kNoMatch},           // sums past 2^64
      {true, 10, ~0ull - 2, 0, false, S::kNoMatch},
      {true, ~0ull, ~0ull, 0, false, S::kNoMatch},
      {false, 0, 0, 0, false, S::kMaskOfZero},                // padding passes: Mask(Value("")) = Mask(0)
      {false, ~0ull, 5, 0, false, S::kMaskOfZero},
  };
  for (const auto& c : cases) {
    const S::Prep p = S::prep(c.real, c.off, c.len, n);
    const bool same = p.len1 == c.len1 && p.read == c.read && (p.read || p.stored == c.stored);
    const bool inside = !p.read || (c.off + c.len + 5 <= n && c.off + c.len + 5 >= c.off);
    if (!same || !inside || S::usable(c.off, c.len, n) != ref_usable(c.off, c.len, n)) {
      printf("FAILED prep rule for (%llu, %llu)\n", (unsigned long long)c.off, (unsigned long long)c.len);
      ++g_failed;
    }
    ++g_cases;
  }
  if (S::kNoMatch == S::kMaskOfZero || S::listed(1, 5, 9) != 0 || S::listed(0, 5, 9) != 7 || S::listed(7, 50, 9) != 9 ||
      S::listed(2, 0, 9) != 2) {
    printf("FAILED listed()\n");
    ++g_failed;
  }
}

}  // namespace

int main() {
  small_blocks();
  tail_mutations();
  restart_counts();
  footers();
  table_form();
  prep_rules();
  for (const Wrong& w : g_wrong) printf("wrong rule (%s): caught in %ld cases\n", w.name, w.caught);
  printf("%ld emulated calls, %ld failed\n", g_cases, g_failed);
  bool all = true;
  for (const Wrong& w : g_wrong) all = all && w.caught > 0;
  if (g_failed || !all) {
    printf("FAIL\n");
    return 1;
  }
  printf("PASS\n");
  return 0;
}
