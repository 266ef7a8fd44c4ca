// sstw_run_test.cc -- the SST table writer's kernels (csrc/crc32c_sstbuild.inc: size, fill, tail) run lane by lane on
// the CPU over a memory model, every decision taken from csrc/sstw_run.h, against BlockBuilder::Add / Finish and
// Footer::EncodeTo restated serially.  Checked per emulated call: the block, its trailer (the table form: metaindex
// block and footer too) equal the serial result; every destination byte of the range is written exactly once and none
// outside it; a 16-B store is naturally aligned; every key byte read lies inside a kept key (the unstaged path: inside
// a 16-B granule that holds such a byte); a staged granule is stored only when all its bytes were staged; a refusal
// writes nothing.  Three deliberately wrong rules must be caught.  Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pack_run.h"
#include "sstw_run.h"

using namespace kvsep;

namespace {

uint64_t g_calls = 0, g_failed = 0;
bool g_quiet = false;
uint64_t g_caught = 0;
void fail(const std::string& what) {
  ++g_failed;
  if (!g_quiet && g_failed < 20) printf("FAIL: %s\n", what.c_str());
}

// ---- CRC-32C, bit by bit (util/crc32c.cc gives the same values)
uint32_t crc32c(uint32_t crc, const uint8_t* p, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0x82f63b78u & (0u - (crc & 1)));
  }
  return ~crc;
}
uint32_t mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// ---- the serial restatement
void put_varint(std::vector<uint8_t>& b, uint64_t v) {
  while (v >= 128) {
    b.push_back(uint8_t(v | 128));
    v >>= 7;
  }
  b.push_back(uint8_t(v));
}
void put_le32(std::vector<uint8_t>& b, uint32_t v) {
  for (int k = 0; k < 4; ++k) b.push_back(uint8_t(v >> (8 * k)));
}
void put_trailer(std::vector<uint8_t>& out, const std::vector<uint8_t>& blk) {
  const uint8_t type = 0;
  const uint32_t c = crc32c(crc32c(0, blk.data(), blk.size()), &type, 1);
  out.push_back(0);
  put_le32(out, mask(c));
}

struct Case {
  std::vector<uint8_t> src;
  std::vector<uint64_t> ko, kl, bo, bl;
  std::vector<uint8_t> keep;
  bool has_keep = true;
  uint64_t at = 0, dst_bytes = 0, skew = 0;  // skew: the destination pointer's address mod 16
  uint64_t src_skew = 0;                     // ... and the key source's
  bool table = false;
  uint64_t count() const { return ko.size(); }
  bool kept(uint64_t i) const { return (has_keep ? keep[i] != 0 : true) && bo[i] != ~uint64_t(0); }
};

// BlockBuilder at block_restart_interval = 1 (table/block_builder.cc): restarts_ = {0}, counter_ = 0; Add pushes a
// restart when counter_ >= 1 and then shares nothing; Finish appends the restarts and their count.
std::vector<uint8_t> serial_block(const Case& c) {
  std::vector<uint8_t> buf;
  std::vector<uint32_t> restarts{0};
  int counter = 0;
  for (uint64_t i = 0; i < c.count(); ++i) {
    if (!c.kept(i)) continue;
    if (counter >= 1) {
      restarts.push_back(uint32_t(buf.size()));
      counter = 0;
    }
    std::vector<uint8_t> val;
    put_varint(val, c.bo[i]);
    put_varint(val, c.bl[i]);
    put_varint(buf, 0);
    put_varint(buf, c.kl[i]);
    put_varint(buf, val.size());
    buf.insert(buf.end(), c.src.begin() + c.ko[i], c.src.begin() + c.ko[i] + c.kl[i]);
    buf.insert(buf.end(), val.begin(), val.end());
    ++counter;
  }
  for (uint32_t r : restarts) put_le32(buf, r);
  put_le32(buf, uint32_t(restarts.size()));
  return buf;
}
// What the call writes from `at` on: the block and its trailer; the table form: the empty block framed, the index block
// framed, Footer::EncodeTo.
std::vector<uint8_t> serial_output(const Case& c, uint64_t* block_len) {
  const std::vector<uint8_t> blk = serial_block(c);
  *block_len = blk.size();
  std::vector<uint8_t> out;
  if (c.table) {
    Case none;
    const std::vector<uint8_t> meta = serial_block(none);
    out = meta;
    put_trailer(out, meta);
  }
  out.insert(out.end(), blk.begin(), blk.end());
  put_trailer(out, blk);
  if (c.table) {
    std::vector<uint8_t> f;
    put_varint(f, c.at);
    put_varint(f, 8);
    put_varint(f, c.at + 13);
    put_varint(f, blk.size());
    f.resize(40, 0);
    for (int k = 0; k < 8; ++k) f.push_back(uint8_t(sstw::kMagic >> (8 * k)));
    out.insert(out.end(), f.begin(), f.end());
  }
  return out;
}

// ---- the memory model
struct Mem {
  const Case& c;
  std::vector<uint8_t> dst;
  std::vector<uint32_t> writes;
  std::vector<uint8_t> key_byte, key_gran;  // source bytes inside a kept key; bytes of granules that hold one
  explicit Mem(const Case& cs) : c(cs), dst(cs.dst_bytes, 0xEE), writes(cs.dst_bytes, 0) {
    key_byte.assign(c.src.size(), 0);
    key_gran.assign(c.src.size() + 48, 0);
    for (uint64_t i = 0; i < c.count(); ++i) {
      if (!c.kept(i)) continue;
      for (uint64_t j = 0; j < c.kl[i]; ++j) {
        key_byte[c.ko[i] + j] = 1;
        const uint64_t a = (s0() + c.ko[i] + j) & ~uint64_t(15);  // the granule, as an address
        for (uint64_t k = 0; k < 16; ++k) key_gran[a + k - (s0() - 16)] = 1;
      }
    }
  }
  // addresses: the destination starts at address (1 << 20) + skew
  uint64_t d0() const { return (uint64_t(1) << 20) + c.skew; }
  void st8(uint64_t addr, uint8_t v) {
    const uint64_t o = addr - d0();
    if (addr < d0() || o >= dst.size()) return fail("a byte store outside the destination");
    dst[o] = v;
    ++writes[o];
  }
  void st16(uint64_t addr, const uint8_t* v) {
    if (addr & 15) return fail("a 16-B store that is not naturally aligned");
    for (int k = 0; k < 16; ++k) st8(addr + k, v[k]);
  }
  uint8_t ld_key(uint64_t off) {
    if (off >= c.src.size() || !key_byte[off]) {
      fail("a key byte read outside every kept key");
      return 0;
    }
    return c.src[off];
  }
  // the key source starts at address (1 << 30) + src_skew
  uint64_t s0() const { return (uint64_t(1) << 30) + c.src_skew; }
  uint8_t ld_gran(uint64_t addr) {  // the unstaged path's body loads: a byte of a whole aligned granule
    const uint64_t i = addr - (s0() - 16);  // key_gran starts a granule before the source
    if (addr < s0() - 16 || i >= key_gran.size() || !key_gran[i]) {
      fail("a granule read that holds no kept key byte");
      return 0;
    }
    return addr >= s0() && addr - s0() < c.src.size() ? c.src[addr - s0()] : 0;
  }
};

struct Result {
  uint64_t out_len = ~0ull, table_bytes = ~0ull;
  uint32_t status = ~0u;
};

// ---- the kernels, lane by lane
template <class R>
Result emulate(const Case& c, Mem& m) {
  const uint64_t n = c.count();
  // sstw_size_kernel
  std::vector<uint64_t> size(n), flag(n), pos(n), rank(n);
  for (uint64_t i = 0; i < n; ++i) {
    const bool keep = sstw::kept(c.has_keep ? c.keep[i] : uint8_t(1), c.bo[i]);
    size[i] = sstw::entry_size(keep, c.kl[i], c.bo[i], c.bl[i]);
    flag[i] = keep;
  }
  // the offsets pass, twice (tests/cpp/offsets_run_test.cc runs its kernels): exclusive saturated sums
  uint64_t entries = 0, nkept = 0;
  for (uint64_t i = 0; i < n; ++i) {
    pos[i] = entries, rank[i] = nkept;
    entries = sstw::add_sat(entries, size[i]);
    nkept += flag[i];
  }
  const uint64_t lead = c.table ? sstw::kMetaFramed : 0, trail = c.table ? sstw::kFooter : 0;
  const sstw::Plan p = sstw::plan<R>(entries, nkept, c.at, lead, trail, c.dst_bytes, 0);
  uint64_t crc_off = 0, crc_len = 0;
  // sstw_fill_kernel
  for (uint64_t wg = 0; wg < sstw::grid_for(n); ++wg) {
    for (uint32_t wv = 0; wv < sstw::kWaves; ++wv) {
      const uint64_t i0 = wg * sstw::kThreads + wv * sstw::kWaveLanes;
      if (i0 == 0) crc_off = p.at, crc_len = p.len;
      const bool go = p.status == sstw::kOk;
      const uint64_t d0 = m.d0() + p.at;
      bool mine[64];
      uint64_t kept = 0;
      for (uint32_t l = 0; l < 64; ++l) {
        mine[l] = go && i0 + l < n && flag[i0 + l];
        if (mine[l]) kept |= uint64_t(1) << l;
      }
      uint64_t w0 = 0, len = 0;
      if (kept) {
        const uint64_t f = i0 + __builtin_ctzll(kept), last = i0 + 63 - __builtin_clzll(kept);
        w0 = pos[f];
        len = pos[last] + size[last] - w0;
      }
      const bool staged = kept && sstw::stages(len);
      const uint32_t phase = uint32_t((d0 + w0) & (sstw::kGran - 1));
      std::vector<uint8_t> stage(sstw::kStageGranules * sstw::kGran, 0), set(stage.size(), 0);
      auto put = [&](uint64_t o, uint8_t v) {
        if (phase + o >= stage.size()) return fail("a stage byte past the staging area");
        if (set[phase + o]) fail("a stage byte written twice");
        stage[phase + o] = v, set[phase + o] = 1;
      };
      if (staged)
        for (uint32_t l = 0; l < 64; ++l) {
          if (!mine[l]) continue;
          const uint64_t i = i0 + l, e = pos[i] - w0, kl = c.kl[i];
          const uint32_t h = sstw::head_len(kl), vl = sstw::value_len(c.bo[i], c.bl[i]);
          for (uint32_t j = 0; j < h; ++j) put(e + j, sstw::head_byte(j, kl, vl));
          for (uint64_t j = 0; j < kl; ++j) put(e + h + j, m.ld_key(c.ko[i] + j));
          for (uint32_t j = 0; j < vl; ++j) put(e + h + kl + j, sstw::value_byte(j, c.bo[i], c.bl[i]));
        }
      // __syncthreads()
      if (staged) {
        const uint64_t d = d0 + w0;
        const sstw::Span s = sstw::split<R>(d, len);
        for (uint32_t l = 0; l < 64; ++l)
          if (l < s.head + s.tail) {
            const uint64_t e = sstw::edge_index(s, len, l);
            if (phase + e >= stage.size() || !set[phase + e]) fail("an edge byte that was not staged");
            else m.st8(d + e, stage[phase + e]);
          }
        const uint64_t g0 = (phase + s.head) / sstw::kGran;
        for (uint64_t g = 0; g < s.body; ++g) {
          const uint64_t o = (g0 + g) * sstw::kGran;
          bool whole = o + 16 <= stage.size();
          for (int k = 0; whole && k < 16; ++k) whole = set[o + k];
          if (!whole) fail("a granule stored that was not staged whole");
          else m.st16(d + s.head + g * sstw::kGran, &stage[o]);
        }
      } else {
        for (uint64_t todo = kept; todo; todo &= todo - 1) {
          const uint64_t i = i0 + __builtin_ctzll(todo), kl = c.kl[i];
          const uint32_t h = sstw::head_len(kl), vl = sstw::value_len(c.bo[i], c.bl[i]);
          for (uint32_t l = 0; l < 64; ++l)
            if (l < h + vl) {
              const uint64_t j = l < h ? l : l + kl;
              m.st8(d0 + pos[i] + j, sstw::frame_byte(j, kl, c.bo[i], c.bl[i]));
            }
          if (kl) {  // crc32c_pack.inc's pack_span, from pack_run.h: byte loads at the edges, granule loads in the body
            const uint64_t src = m.s0() + c.ko[i];
            const pack::Span s = pack::split(src, d0 + pos[i] + h, kl);
            for (uint32_t l = 0; l < 64; ++l) {
              const uint64_t e = pack::edge_byte(s, l);
              if (e != ~uint64_t(0)) m.st8(s.dst + e, m.ld_key(c.ko[i] + e));
            }
            for (uint64_t it = 0; it < pack::body_iters(s); ++it)
              for (uint32_t u = 0; u < pack::kUnroll; ++u)
                for (uint32_t l = 0; l < 64; ++l) {
                  const uint64_t g = pack::body_granule(s, it, u, l);
                  if (!g) continue;
                  const uint64_t a = pack::body_src(s, g);
                  uint8_t both[32] = {0}, v[16];
                  for (int k = 0; k < 16; ++k) both[k] = m.ld_gran(a + k);
                  if (s.sh)
                    for (int k = 0; k < 16; ++k) both[16 + k] = m.ld_gran(a + 16 + k);
                  for (int k = 0; k < 16; ++k) v[k] = both[s.sh + k];
                  m.st16(g, v);
                }
          }
        }
      }
      for (uint32_t l = 0; l < 64; ++l)
        if (mine[l]) {
          const uint64_t i = i0 + l, r = d0 + sstw::restart_at<R>(entries, rank[i], i);
          for (uint32_t j = 0; j < 4; ++j) m.st8(r + j, uint8_t(uint32_t(pos[i]) >> (8 * j)));
        }
      if (go && i0 == 0) {
        const uint64_t ca = d0 + sstw::count_at<R>(entries, nkept);
        for (uint32_t j = 0; j < 4; ++j) m.st8(ca + j, uint8_t(sstw::count_word<R>(nkept) >> (8 * j)));
        if (sstw::lone_restart<R>(nkept))
          for (uint32_t j = 0; j < 4; ++j) m.st8(d0 + entries + j, 0);
      }
    }
  }
  // the batched checksum over [crc_off, + crc_len), then sstw_tail_kernel
  uint32_t crc = 0;
  if (crc_len && crc_off + crc_len <= m.dst.size()) crc = crc32c(0, m.dst.data() + crc_off, crc_len);
  const uint8_t type = 0;
  const uint32_t masked = mask(crc32c(crc, &type, 1));
  Result r;
  r.out_len = p.need, r.status = p.status, r.table_bytes = sstw::table_bytes(p);
  if (p.status != sstw::kOk) return r;
  const uint64_t t = m.d0() + p.at + p.len;
  uint8_t meta[9];
  for (uint32_t j = 0; j < 9; ++j) meta[j] = sstw::meta_byte(j, 0);
  const uint32_t meta_masked = mask(crc32c(0, meta, 9));
  for (uint32_t l = 0; l < sstw::kTailThreads; ++l) {
    if (l < sstw::kTrailer) m.st8(t + l, sstw::trailer_byte(l, masked));
    if (!c.table) continue;
    if (l < sstw::kMetaFramed) m.st8(m.d0() + c.at + l, sstw::meta_byte(l, meta_masked));
    if (l < sstw::kFooter) m.st8(t + sstw::kTrailer + l, sstw::footer_byte(l, c.at, sstw::kEmptyBlock, p.at, p.len));
  }
  return r;
}

template <class R>
void check(const Case& c, const std::string& what) {
  ++g_calls;
  const uint64_t before = g_failed;
  uint64_t blen = 0;
  const std::vector<uint8_t> want = serial_output(c, &blen);
  const bool room = c.at <= c.dst_bytes && want.size() <= c.dst_bytes - c.at;
  Mem m(c);
  const Result r = emulate<R>(c, m);
  if (!room) {
    if (r.status != sstw::kNoRoom || r.out_len != blen || r.table_bytes != 0) fail(what + ": the no-room report");
    for (uint32_t w : m.writes)
      if (w) {
        fail(what + ": a refused call wrote");
        break;
      }
  } else {
    if (r.status != sstw::kOk || r.out_len != blen) fail(what + ": status or out_len");
    if (c.table && r.table_bytes != c.at + want.size()) fail(what + ": table_bytes");
    for (uint64_t o = 0; o < m.dst.size(); ++o) {
      const bool in = o >= c.at && o - c.at < want.size();
      if (m.writes[o] != (in ? 1u : 0u)) {
        fail(what + ": destination byte " + std::to_string(o) + " written " + std::to_string(m.writes[o]) + " times");
        break;
      }
      if (in && m.dst[o] != want[o - c.at]) {
        fail(what + ": byte " + std::to_string(o - c.at) + " of the output differs from the serial BlockBuilder");
        break;
      }
    }
  }
  if (g_failed != before) ++g_caught;
}

uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
  return rnd_state;
}

Case make(uint64_t count, int mask_kind, const std::vector<uint64_t>& klens, const std::vector<uint64_t>& vals) {
  Case c;
  uint64_t total = 0;
  for (uint64_t i = 0; i < count; ++i) total += klens[i % klens.size()] + 3;
  c.src.resize(total + 7);
  for (auto& b : c.src) b = uint8_t(rnd());
  uint64_t p = 5;
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t k = klens[i % klens.size()];
    c.ko.push_back(p), c.kl.push_back(k);
    p += k + (i % 3);
    c.bo.push_back(vals[i % vals.size()]);
    c.bl.push_back(vals[(5 * i + 2) % vals.size()]);
    uint8_t keep = 1;
    switch (mask_kind) {
      case 0: keep = 0; break;
      case 1: keep = 1; break;
      case 2: keep = i & 1; break;
      case 3: keep = i == 0; break;
      case 4: keep = i + 1 == count; break;
      default:  // kSkip handles mixed with keep
        keep = i % 3 != 0;
        if (i % 4 == 1) c.bo.back() = ~uint64_t(0);
    }
    c.keep.push_back(keep);
  }
  if (mask_kind == 1) c.has_keep = false;
  return c;
}

template <class R>
void suite() {
  const std::vector<uint64_t> small{21}, vals_small{0, 4101, 8202, 1ull << 20};
  std::vector<uint64_t> widths{0, 1};
  for (int b = 7; b < 64; b += 7) widths.push_back((1ull << b) - 1), widths.push_back(1ull << b);
  widths.push_back(1ull << 63), widths.push_back(~uint64_t(0) - 1);
  auto place = [](Case& c, uint64_t at, uint64_t skew, bool table, int64_t slack) {
    uint64_t blen;
    c.at = at, c.skew = skew, c.table = table;
    c.dst_bytes = 0;
    c.dst_bytes = uint64_t(int64_t(at + serial_output(c, &blen).size()) + slack);
  };
  // counts at row and tile edges under every keep mask, both forms
  for (uint64_t count : std::vector<uint64_t>{0, 1, 63, 64, 65, 1024, 1025})
    for (int mk = 0; mk < 6; ++mk)
      for (int table = 0; table < 2; ++table) {
        Case c = make(count, mk, small, vals_small);
        place(c, 7 + count % 5, count % 16, table, 9);
        check<R>(c, "count " + std::to_string(count) + " mask " + std::to_string(mk) + (table ? " table" : ""));
      }
  // key lengths across the two-byte non_shared and the staging threshold; handles across every varint width
  {
    Case c = make(3 * widths.size(), 5, {0, 1, 127, 128, sstw::kStageBytes + 1, 16384, 20}, widths);
    place(c, 3, 11, false, 5);
    check<R>(c, "key lengths and handle widths");
    Case d = make(2 * widths.size(), 1, {0, 1, 127, 128, 20, 33}, widths);
    place(d, 1, 2, true, 0);
    check<R>(d, "handle widths, staged");
  }
  // all 16 x 16 alignments of the position and of the key source
  for (uint64_t a = 0; a < 16; ++a)
    for (uint64_t s = 0; s < 16; ++s) {
      Case c = make(5, 1, {20, 130, sstw::kStageBytes + 1, 17, 64}, vals_small);
      for (auto& o : c.ko) o += s;
      c.src.resize(c.src.size() + 16, 0x5a);
      c.src_skew = (s * 7) % 16;
      place(c, a, (a * 5 + s) % 16, false, 3);
      check<R>(c, "alignment " + std::to_string(a) + " x " + std::to_string(s));
      Case e = make(70, 2, {20, 21, 19}, vals_small);
      for (auto& o : e.ko) o += s;
      e.src.resize(e.src.size() + 16, 0x5a);
      place(e, a, s, true, 0);
      check<R>(e, "staged alignment " + std::to_string(a) + " x " + std::to_string(s));
    }
  // the room: exactly enough, one short, far short
  for (int64_t slack : std::vector<int64_t>{0, -1, -40})
    for (int table = 0; table < 2; ++table) {
      Case c = make(66, 2, small, vals_small);
      place(c, 29, 3, table, slack);
      check<R>(c, "slack " + std::to_string(slack));
    }
}

struct NoEmptyRestart : sstw::Rule {
  static uint64_t restarts(uint64_t nkept) { return nkept; }
};
struct RankFromIndex : sstw::Rule {
  static uint64_t slot(uint64_t, uint64_t index) { return index; }
};
struct EdgeInGranule : sstw::Rule {
  static uint64_t body_begin(uint64_t d) { return d & ~uint64_t(sstw::kGran - 1); }
};

template <class R>
void planted(const char* name) {
  const uint64_t failed = g_failed, calls = g_calls;
  g_quiet = true, g_caught = 0;
  suite<R>();
  g_quiet = false;
  printf("wrong rule (%s): caught in %llu cases\n", name, (unsigned long long)g_caught);
  g_failed = failed, g_calls = calls;
}

// The refusals from the totals alone: sizes faked through the pure functions, nothing allocated.
void pure() {
  auto expect = [](bool ok, const char* what) {
    if (!ok) fail(what);
  };
  using sstw::plan;
  const uint64_t M = ~uint64_t(0);
  expect(sstw::entry_size(true, 1ull << 32, 0, 0) == sstw::kSaturated, "a key_len over 2^32 - 1 saturates");
  expect(sstw::entry_size(true, 0xffffffffull, 0, 0) == 0xffffffffull + 7 + 2, "the longest key's entry");
  expect(plan(M, 1, 0, 0, 0, M, 0).status == sstw::kTooLarge && plan(M, 1, 0, 0, 0, M, 0).need == 0, "saturated sum");
  // block_len = entries + 4 * nkept + 4: 2^32 - 1 is the last that fits
  expect(plan((1ull << 32) - 1 - 8, 1, 0, 0, 0, M, 0).status == sstw::kOk, "a block of 2^32 - 1 bytes");
  expect(plan((1ull << 32) - 8, 1, 0, 0, 0, M, 0).status == sstw::kTooLarge, "a block of 2^32 bytes");
  const uint64_t len = 100 + 4 + 4;
  expect(plan(100, 1, 50, 0, 0, 50 + len + 5, 0).status == sstw::kOk, "at + len + 5 == dst_bytes");
  expect(plan(100, 1, 50, 0, 0, 50 + len + 4, 0).status == sstw::kNoRoom, "at + len + 5 == dst_bytes + 1");
  expect(plan(100, 1, 50, 0, 0, 50 + len + 4, 0).need == len, "the needed length of a block with no room");
  expect(plan(100, 1, M - 3, 0, 0, M, 0).status == sstw::kNoRoom, "at + len + 5 past 2^64");
  expect(plan(100, 1, M, 0, 0, 10, 0).status == sstw::kNoRoom, "at past dst_bytes");
  expect(plan(100, 1, 50, 13, 48, 50 + 13 + len + 5 + 48, 0).status == sstw::kOk, "the table form's room");
  expect(plan(100, 1, 50, 13, 48, 50 + 13 + len + 5 + 47, 0).status == sstw::kNoRoom, "the table form, one short");
  for (uint32_t st : {1u, 2u, 3u, 8u}) expect(plan(100, 1, 0, 13, 48, M, st).status == sstw::kSource, "a source refusal");
  for (uint32_t st : {0u, 4u, 5u, 6u, 7u}) expect(plan(100, 1, 0, 13, 48, M, st).status == sstw::kOk, "a later entry error");
  expect(sstw::table_bytes(plan(100, 1, 0, 13, 48, 10, 0)) == 0, "table_bytes after a refusal");
  for (uint64_t v : std::vector<uint64_t>{0, 127, 128, 16383, 16384, 1ull << 63, M}) {
    std::vector<uint8_t> b;
    put_varint(b, v);
    expect(sstw::varint_len(v) == b.size(), "varint_len");
    for (uint32_t k = 0; k < b.size(); ++k) expect(sstw::varint_byte(v, k) == b[k], "varint_byte");
  }
  expect(sstw::scratch_words(0) == sstw::kWords && sstw::scratch_words(9) == 36 + 2 + sstw::kWords, "scratch_words");
}

}  // namespace

int main() {
  pure();
  suite<sstw::Rule>();
  printf("%llu emulated calls, %llu failed\n", (unsigned long long)g_calls, (unsigned long long)g_failed);
  const uint64_t failed = g_failed;
  planted<NoEmptyRestart>("a restart array with no entry for the empty block");
  planted<RankFromIndex>("a rank taken from the entry index");
  planted<EdgeInGranule>("an edge written with a 16-B store");
  puts(failed ? "FAIL" : "PASS");
  return failed ? 1 : 0;
}
