// offsets_run_test.cc -- the geometry of the offsets pass (csrc/offsets_run.h) on the CPU, no GPU and no library.
//
// emulate() below is the control flow of the three kernels of csrc/crc32c_offsets.inc written lane by lane over a
// memory model: every workgroup, wave, row and lane of offsets_tile_sum_kernel (the serial sums of short runs, the
// wave-uniform loop over a row's long runs, the wave scan that reduces them), the 256 threads of
// offsets_tile_scan_kernel with their LDS scan, and offsets_write_kernel's row scans, row and wave chaining.  Every
// index and arithmetic decision is a call into offsets_run.h, the header the kernels themselves include.  Per launch:
//   * dst_off, *end and *nkept equal a plain serial loop written from the contract alone;
//   * dst_off is written exactly once per block and nothing around it, *end and *nkept exactly once;
//   * seg_len is read at indices < nseg only and only inside kept blocks' clamped runs, first for count + 1 elements,
//     keep for count;
//   * every scratch word read was written earlier in the same launch (a replay reads nothing stale).
// Three deliberately wrong rules (an inclusive scan, the keep mask ignored in the tile total, an unclamped first[])
// must each be caught.  Built with -fsanitize=address,undefined by tests/test_offsets_run_cpu.py and run as it is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "offsets_run.h"
#include "pack_run.h"

using namespace kvsep;

namespace {

constexpr uint64_t kMax = ~uint64_t(0);
constexpr uint64_t kCanary = 0xC0FFEE1234567ull;
constexpr uint64_t kPad = 3;  // canary words on each side of dst_off

long g_failed = 0, g_cases = 0;
std::string g_case;

struct Batch {
  std::vector<uint64_t> seg_len, first;
  bool identity = true;  // no first[]: block i is segment i
  std::vector<uint8_t> keep;
  bool has_keep = false, has_before = false;
  uint64_t before = kMax;
  uint64_t head = 0, tail = 0, start = 0, max_size = kMax;
  uint64_t count = 0;
  bool want_nkept = true;
};

struct Rules {
  bool inclusive = false;         // wrong: the block's own extent is not taken off its end
  bool mask_free_total = false;   // wrong: a dropped block still adds to its tile's total
  bool unclamped_first = false;   // wrong: first[] used as it comes
};

struct Word {
  uint64_t v = 0;
  bool set = false;
};

struct Model {
  const Batch& b;
  long problems = 0;
  bool quiet;
  std::vector<uint64_t> dst_off;
  std::vector<uint8_t> writes;
  uint64_t end = kCanary, nkept = kCanary;
  int end_writes = 0, nkept_writes = 0;
  std::vector<Word> ext, tile_sum, tile_kept, tile_base, grand;
  std::vector<uint8_t> seg_allowed;

  Model(const Batch& batch, bool q) : b(batch), quiet(q), dst_off(batch.count + 2 * kPad, kCanary),
                                      writes(batch.count + 2 * kPad, 0), seg_allowed(batch.seg_len.size(), 0) {
    const uint64_t nt = offsets::tile_count(b.count);
    ext.resize(b.count), tile_sum.resize(nt), tile_kept.resize(nt), tile_base.resize(nt), grand.resize(2);
    // the segments a correct pass may read: the clamped runs of the kept blocks
    const uint64_t nseg = b.seg_len.size();
    for (uint64_t i = 0; i < b.count; ++i) {
      if (!ref_kept(i)) continue;
      uint64_t s = b.identity ? i : b.first[i], e = b.identity ? i + 1 : b.first[i + 1];
      if (s > nseg) s = nseg;
      if (e > nseg) e = nseg;
      for (uint64_t j = s; j < e; ++j) seg_allowed[j] = 1;
    }
  }
  void bad(const char* what, uint64_t x = 0, uint64_t y = 0) {
    if (!quiet && g_failed + problems < 20)
      printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)x, (unsigned long long)y);
    ++problems;
  }
  bool ref_kept(uint64_t i) const {
    if (b.has_keep) return b.keep[i] != 0;
    if (b.has_before) return i < b.before;
    return true;
  }
  uint64_t first_at(uint64_t i) {
    if (i > b.count || i >= b.first.size()) { bad("first[] read past count + 1 elements", i); return 0; }
    return b.first[i];
  }
  uint64_t len_at(uint64_t j) {
    if (j >= b.seg_len.size()) { bad("a segment index >= nseg was read", j); return 0; }
    if (!seg_allowed[j]) bad("a segment outside the kept blocks' runs was read", j);
    return b.seg_len[j];
  }
  uint8_t keep_at(uint64_t i) {
    if (i >= b.count) { bad("keep[] read past count elements", i); return 0; }
    return b.keep[i];
  }
  uint64_t rd(std::vector<Word>& a, uint64_t i, const char* what) {
    if (i >= a.size()) { bad(what, i); return 0; }
    if (!a[i].set) bad("a scratch word read before this launch wrote it", i);
    return a[i].v;
  }
  void wr(std::vector<Word>& a, uint64_t i, uint64_t v, const char* what) {
    if (i >= a.size()) { bad(what, i); return; }
    a[i] = {v, true};
  }
  void put(uint64_t i, uint64_t v) {
    if (i >= b.count) { bad("dst_off written past count elements", i); return; }
    dst_off[kPad + i] = v;
    ++writes[kPad + i];
  }
};

// offsets_wave_scan over the 64 lanes' values
void wave_scan(uint64_t (&v)[64]) {
  for (uint32_t step = 0; step < offsets::kScanSteps; ++step) {
    const uint32_t n = offsets::scan_shift(step);
    uint64_t nv[64];
    for (uint32_t l = 0; l < 64; ++l) {
      // DPP row_shr:n -- lane l - n of the same 16-lane row, 0 where the row has none
      const uint64_t left = (l & 15u) >= n ? v[l - n] : 0;
      nv[l] = offsets::add_sat(v[l], offsets::scan_takes(l, n) ? left : 0);
    }
    for (uint32_t l = 0; l < 64; ++l) v[l] = nv[l];
  }
  const uint64_t t15 = v[15], t31 = v[31], t47 = v[47];
  for (uint32_t l = 0; l < 64; ++l) v[l] = offsets::add_sat(v[l], offsets::row_base(l, t15, t31, t47));
}

bool kept_of(Model& m, uint64_t before, uint64_t i) {
  return offsets::is_kept(m.b.has_keep ? m.keep_at(i) : uint8_t(1), before, i);
}

void emulate_tile_sum(Model& m, const Rules& rules) {
  const Batch& b = m.b;
  const uint64_t nseg = b.seg_len.size(), nt = offsets::tile_count(b.count);
  const uint64_t before = b.has_before ? b.before : offsets::kKeepAll;
  for (uint64_t tile = 0; tile < nt; ++tile) {
    uint64_t ws[offsets::kWaves], wk[offsets::kWaves];
    for (uint32_t w = 0; w < offsets::kWaves; ++w) {
      uint64_t mine[64] = {0};
      uint64_t nk = 0;
      for (uint32_t row = 0; row < offsets::kRows; ++row) {
        offsets::Run r[64];
        bool own[64], kept[64], is_long[64];
        uint64_t sum[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t i = offsets::block_index(tile, w, row, lane);
          own[lane] = i < b.count;
          r[lane] = {0, 0};
          kept[lane] = false;
          sum[lane] = 0;
          if (own[lane]) {
            kept[lane] = kept_of(m, before, i);
            if (b.identity) r[lane] = offsets::clamp_run(i, i + 1, nseg);
            else if (rules.unclamped_first) r[lane] = {m.first_at(i), m.first_at(i + 1)};
            else r[lane] = offsets::clamp_run(m.first_at(i), m.first_at(i + 1), nseg);
          }
          const bool sums = rules.mask_free_total ? own[lane] : kept[lane];
          is_long[lane] = sums && !offsets::is_short(r[lane]);
          if (sums && !is_long[lane])
            for (uint64_t j = r[lane].s; j < r[lane].e && j - r[lane].s <= concat::kShortMax; ++j)
              sum[lane] = offsets::add_sat(sum[lane], m.len_at(j));
        }
        for (uint32_t src = 0; src < 64; ++src) {  // the ballot's bits, lowest first
          if (!is_long[src]) continue;
          const offsets::Run run = r[src];
          uint64_t iters = offsets::long_iters(run);
          if (iters > 64) iters = 64;  // (only a wrong rule gets here: keep its run time bounded)
          uint64_t part[64] = {0};
          for (uint64_t k = 0; k < iters; ++k)
            for (uint32_t lane = 0; lane < 64; ++lane) {
              const uint64_t j = offsets::long_seg(run, k, lane);
              if (j != kMax) part[lane] = offsets::add_sat(part[lane], m.len_at(j));
            }
          wave_scan(part);
          sum[src] = part[63];
        }
        for (uint32_t lane = 0; lane < 64; ++lane) {
          if (own[lane]) {
            const bool adds = rules.mask_free_total ? true : kept[lane];
            const uint64_t ext = offsets::extent(adds, b.head, offsets::block_size(sum[lane], b.max_size), b.tail);
            m.wr(m.ext, offsets::block_index(tile, w, row, lane), ext, "ext[] written past count");
            mine[lane] = offsets::add_sat(mine[lane], ext);
          }
          nk += kept[lane] ? 1 : 0;
        }
      }
      wave_scan(mine);
      ws[w] = mine[63];
      wk[w] = nk;
    }
    uint64_t s = 0, k = 0;
    for (uint32_t w = 0; w < offsets::kWaves; ++w) s = offsets::add_sat(s, ws[w]), k += wk[w];
    m.wr(m.tile_sum, tile, s, "tile_sum[] written past the tiles");
    m.wr(m.tile_kept, tile, k, "tile_kept[] written past the tiles");
  }
}

void emulate_tile_scan(Model& m) {
  const uint64_t nt = offsets::tile_count(m.b.count);
  constexpr uint32_t T = offsets::kScanThreads;
  std::vector<uint64_t> sh(T), shk(T);
  const uint64_t run = offsets::scan_run(nt);
  std::vector<uint8_t> covered(nt, 0);
  for (uint32_t t = 0; t < T; ++t) {
    const offsets::Run r = offsets::scan_range(t, run, nt);
    uint64_t s = 0, k = 0;
    for (uint64_t i = r.s; i < r.e; ++i) {
      s = offsets::add_sat(s, m.rd(m.tile_sum, i, "tile_sum[] read past the tiles"));
      k += m.rd(m.tile_kept, i, "tile_kept[] read past the tiles");
      if (i < nt) ++covered[i];
    }
    sh[t] = s, shk[t] = k;
  }
  for (uint64_t i = 0; i < nt; ++i)
    if (covered[i] != 1) m.bad("a tile is in no thread's run, or in two", i, covered[i]);
  for (uint32_t d = 1; d < T; d <<= 1) {
    std::vector<uint64_t> v(T), vk(T);
    for (uint32_t t = 0; t < T; ++t) v[t] = t >= d ? sh[t - d] : 0, vk[t] = t >= d ? shk[t - d] : 0;
    for (uint32_t t = 0; t < T; ++t) sh[t] = offsets::add_sat(sh[t], v[t]), shk[t] += vk[t];
  }
  for (uint32_t t = 0; t < T; ++t) {
    const offsets::Run r = offsets::scan_range(t, run, nt);
    uint64_t at = t ? sh[t - 1] : 0;
    for (uint64_t i = r.s; i < r.e; ++i) {
      const uint64_t v = m.rd(m.tile_sum, i, "tile_sum[] read past the tiles");
      m.wr(m.tile_base, i, at, "tile_base[] written past the tiles");
      at = offsets::add_sat(at, v);
    }
  }
  m.wr(m.grand, 0, sh[T - 1], "grand");
  m.wr(m.grand, 1, shk[T - 1], "grand");
}

void emulate_write(Model& m, const Rules& rules) {
  const Batch& b = m.b;
  if (b.count == 0) {
    m.end = offsets::layout_end(b.start, 0), ++m.end_writes;
    if (b.want_nkept) m.nkept = 0, ++m.nkept_writes;
    return;
  }
  const uint64_t nt = offsets::tile_count(b.count);
  const uint64_t before = b.has_before ? b.before : offsets::kKeepAll;
  for (uint64_t tile = 0; tile < nt; ++tile) {
    const uint64_t base = m.rd(m.tile_base, tile, "tile_base[] read past the tiles");
    uint64_t g_total = 0, g_kept = 0;
    if (tile == 0) g_total = m.rd(m.grand, 0, "grand"), g_kept = m.rd(m.grand, 1, "grand");
    uint64_t ws[offsets::kWaves];
    uint64_t v[offsets::kWaves][offsets::kRows][64], inc[offsets::kWaves][offsets::kRows][64];
    bool kept[offsets::kWaves][offsets::kRows][64];
    for (uint32_t w = 0; w < offsets::kWaves; ++w) {
      for (uint32_t row = 0; row < offsets::kRows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t i = offsets::block_index(tile, w, row, lane);
          v[w][row][lane] = 0, kept[w][row][lane] = false;
          if (i < b.count) {
            v[w][row][lane] = m.rd(m.ext, i, "ext[] read past count");
            kept[w][row][lane] = kept_of(m, before, i);
          }
        }
      uint64_t carry = 0;
      for (uint32_t row = 0; row < offsets::kRows; ++row) {
        for (uint32_t lane = 0; lane < 64; ++lane) inc[w][row][lane] = v[w][row][lane];
        wave_scan(inc[w][row]);
        const uint64_t tot = inc[w][row][63];
        for (uint32_t lane = 0; lane < 64; ++lane) inc[w][row][lane] = offsets::add_sat(inc[w][row][lane], carry);
        carry = offsets::add_sat(carry, tot);
      }
      ws[w] = carry;
    }
    for (uint32_t w = 0; w < offsets::kWaves; ++w) {
      uint64_t pre = offsets::add_sat(b.start, base);
      for (uint32_t u = 0; u < w; ++u) pre = offsets::add_sat(pre, ws[u]);
      for (uint32_t row = 0; row < offsets::kRows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t i = offsets::block_index(tile, w, row, lane);
          if (i >= b.count) continue;
          const uint64_t e = offsets::add_sat(pre, inc[w][row][lane]);
          m.put(i, rules.inclusive ? offsets::place(kept[w][row][lane], e, 0)
                                   : offsets::place(kept[w][row][lane], e, v[w][row][lane]));
        }
    }
    if (tile == 0) {
      m.end = offsets::layout_end(b.start, g_total), ++m.end_writes;
      if (b.want_nkept) m.nkept = g_kept, ++m.nkept_writes;
    }
  }
}

// The contract, read independently: one serial loop.
void reference(const Batch& b, std::vector<uint64_t>& off, uint64_t& end, uint64_t& nkept) {
  const uint64_t nseg = b.seg_len.size();
  off.assign(b.count, kMax);
  uint64_t pos = b.start;
  nkept = 0;
  for (uint64_t i = 0; i < b.count; ++i) {
    const bool kept = b.has_keep ? b.keep[i] != 0 : b.has_before ? i < b.before : true;
    if (!kept) continue;
    ++nkept;
    uint64_t s = b.identity ? i : b.first[i], e = b.identity ? i + 1 : b.first[i + 1];
    if (s > nseg) s = nseg;
    if (e > nseg) e = nseg;
    unsigned __int128 size = 0;
    for (uint64_t j = s; j < e; ++j) size += b.seg_len[j];  // (a run of < 2^64 segments cannot wrap 128 bits)
    const bool oversize = size > b.max_size;
    const unsigned __int128 endx = (unsigned __int128)pos + b.head + size + b.tail;
    if (oversize || endx >= kMax) {
      pos = kMax;  // this block and every kept one after it: no offset
      continue;
    }
    off[i] = pos;
    pos = uint64_t(endx);
  }
  end = pos;
}

long run_case(const Batch& b, const Rules& rules, bool quiet) {
  Model m(b, quiet);
  if (b.count) {
    emulate_tile_sum(m, rules);
    emulate_tile_scan(m);
  }
  emulate_write(m, rules);
  std::vector<uint64_t> off;
  uint64_t end, nkept;
  reference(b, off, end, nkept);
  for (uint64_t i = 0; i < b.count; ++i) {
    if (m.writes[kPad + i] != 1) m.bad("dst_off[i] not written exactly once", i, m.writes[kPad + i]);
    if (m.dst_off[kPad + i] != off[i]) m.bad("dst_off[i] differs from the serial loop", i, m.dst_off[kPad + i]);
  }
  for (uint64_t k = 0; k < kPad; ++k)
    if (m.dst_off[k] != kCanary || m.dst_off[kPad + b.count + k] != kCanary) m.bad("a word around dst_off was written", k);
  if (m.end_writes != 1 || m.end != end) m.bad("*end", m.end, end);
  if (b.want_nkept ? (m.nkept_writes != 1 || m.nkept != nkept) : (m.nkept_writes != 0 || m.nkept != kCanary))
    m.bad("*nkept", m.nkept, nkept);
  return m.problems;
}

// The cases, each given to `visit`: the whole set runs once under the right rules and once under each wrong one.
template <typename Visit>
void all_cases(Visit visit) {
  std::mt19937_64 rng(20261020);
  const uint64_t alphabet[] = {0, 1, 7, 300, 4096, 70000};
  auto keep_rules = [&](Batch b, const std::string& name) {
    const uint64_t n = b.count;
    for (int mode = 0; mode < 9; ++mode) {
      Batch c = b;
      c.want_nkept = mode != 3;
      switch (mode) {
        case 0: break;  // keep all: neither rule
        case 1: c.has_keep = true, c.keep.assign(n, 1); break;
        case 2: c.has_keep = true, c.keep.assign(n, 0); break;
        case 3: c.has_keep = true, c.keep.resize(n); for (uint64_t i = 0; i < n; ++i) c.keep[i] = uint8_t(i & 1 ? 0x80 : 0); break;
        case 4: c.has_keep = true, c.keep.resize(n); for (uint64_t i = 0; i < n; ++i) c.keep[i] = uint8_t(rng() % 3 == 0 ? 0 : 1 + rng() % 255); break;
        case 5: c.has_before = true, c.before = 0; break;
        case 6: c.has_before = true, c.before = n / 2; break;
        case 7: c.has_before = true, c.before = n; break;
        default: c.has_before = true, c.before = kMax; break;
      }
      visit(c, name + " keep-mode " + std::to_string(mode));
    }
  };
  // every count around the wave and tile edges, block i = segment i, lengths from a small alphabet
  for (uint64_t count = 0; count <= 1030; count = count == 70 ? 1020 : count + 1) {
    Batch b;
    b.count = count;
    b.seg_len.resize(count);
    for (auto& l : b.seg_len) l = alphabet[rng() % 6];
    b.head = count % 3 == 0 ? 8 : 0, b.tail = count % 2 ? 5 : 0, b.start = count % 5 ? 0 : 12345;
    keep_rules(b, "count " + std::to_string(count));
  }
  {  // fewer segments than blocks without first[]: the blocks past nseg are empty
    Batch b;
    b.count = 40, b.seg_len.assign(17, 100), b.tail = 5;
    keep_rules(b, "identity, nseg < count");
  }
  // every first[] over a small alphabet, decreasing and oversized values included (3 blocks, 6 segments)
  {
    const uint64_t fa[] = {0, 1, 2, 5, 6, 7, kMax};
    for (int x = 0; x < 7 * 7 * 7 * 7; ++x) {
      Batch b;
      b.identity = false, b.count = 3;
      b.seg_len = {3, 0, 1000, 17, 1, 70000};
      b.first = {fa[x % 7], fa[x / 7 % 7], fa[x / 49 % 7], fa[x / 343 % 7]};
      b.head = 8;
      b.has_keep = x % 2, b.keep = {1, uint8_t(x % 4 < 2), 1};
      visit(b, "first[] #" + std::to_string(x));
    }
  }
  // runs of 0, 1, 32, 33, 64, 65 and 1,500 segments, several long runs in one row, across a tile edge
  {
    const uint64_t run_len[] = {0, 1, 32, 33, 64, 65, 1500, 33, 40, 0, 31};
    for (uint64_t count : {11ull, 70ull, 1030ull}) {
      Batch b;
      b.identity = false, b.count = count;
      b.first.push_back(0);
      for (uint64_t i = 0; i < count; ++i) b.first.push_back(b.first.back() + run_len[(i * 7 + count) % 11]);
      b.seg_len.resize(b.first.back());
      for (auto& l : b.seg_len) l = alphabet[rng() % 6];
      b.head = 8, b.start = 99;
      keep_rules(b, "runs, count " + std::to_string(count));
    }
  }
  {  // more than 256 tiles: the scan kernel's per-thread runs hold two tiles
    Batch b;
    b.count = 262145;
    b.seg_len.resize(b.count);
    for (auto& l : b.seg_len) l = rng() % 301;
    b.has_keep = true, b.keep.resize(b.count);
    for (auto& k : b.keep) k = uint8_t(rng() % 4 != 0);
    b.tail = 5;
    visit(b, "257 tiles");
  }
  // sums that reach 2^64: the block that crosses is marked, and so is every kept block after it
  {
    const uint64_t big[] = {uint64_t(1) << 63, kMax, kMax - 1, (uint64_t(1) << 63) - 1, 5, 0};
    for (int x = 0; x < 6 * 6 * 6; ++x)
      for (uint64_t start : {uint64_t(0), uint64_t(1), kMax - 5, kMax})
        for (uint64_t count : {uint64_t(3), uint64_t(130)}) {
          Batch b;
          b.count = count, b.start = start;
          b.seg_len.assign(count, 1);
          b.seg_len[0] = big[x % 6], b.seg_len[count / 2] = big[x / 6 % 6], b.seg_len[count - 1] = big[x / 36];
          b.has_keep = x % 3 == 0, b.keep.assign(count, 1);
          if (b.has_keep) b.keep[0] = 0;
          b.tail = x % 2 ? 5 : 0;
          visit(b, "saturation #" + std::to_string(x) + " start " + std::to_string(start));
        }
    Batch b;  // a long run whose lengths wrap, by the wavefront
    b.identity = false, b.count = 2, b.first = {0, 40, 41};
    b.seg_len.assign(41, uint64_t(1) << 60);
    visit(b, "a long run that saturates");
    b.seg_len.assign(41, 7);  // a block over max_size: the vlog header's LE32 length
    b.seg_len[3] = 0xffffffffull, b.max_size = 0xffffffffull, b.head = 8;
    visit(b, "a block over max_size");
    b.seg_len[3] = 0xffffffffull - 39 * 7;
    visit(b, "a block of exactly max_size");
  }
}

// kSkip lies inside no destination: pack::fits refuses it for every length and frame -- with the one exception of an
// empty plain block in a destination of 2^64 - 1 bytes, which fits and writes nothing.
void skip_is_refused() {
  g_case = "kSkip against pack::fits";
  ++g_cases;
  const uint64_t sizes[] = {0, 1, 80, 4096, uint64_t(1) << 40, kMax - 1, kMax};
  for (pack::Frame f : {pack::kPlain, pack::kVlog, pack::kSst})
    for (uint64_t db : sizes)
      for (uint64_t len = 0; len <= 80; ++len) {
        const bool fits = pack::fits(offsets::kSkip, len, f, db);
        const bool empty_at_the_end = db == kMax && len == 0 && f == pack::kPlain;
        if (fits != empty_at_the_end) {
          if (g_failed < 20) printf("FAILED %s: frame %u dst_bytes %llu len %llu\n", g_case.c_str(), unsigned(f), (unsigned long long)db, (unsigned long long)len);
          ++g_failed;
        }
      }
  if (offsets::kSkip != pack::kSaturated || pack::fits(0, offsets::kSaturated, pack::kPlain, kMax)) ++g_failed;
}

}  // namespace

int main() {
  all_cases([](const Batch& b, const std::string& name) {
    g_case = name;
    ++g_cases;
    g_failed += run_case(b, Rules{}, false);
  });
  skip_is_refused();
  // the model must catch each wrong rule somewhere in the same case set
  const char* names[3] = {"an inclusive scan", "the keep mask ignored in the tile total", "an unclamped first[]"};
  for (int w = 0; w < 3; ++w) {
    Rules r;
    r.inclusive = w == 0, r.mask_free_total = w == 1, r.unclamped_first = w == 2;
    long caught = 0;
    all_cases([&](const Batch& b, const std::string&) {
      if (b.count <= 1100) caught += run_case(b, r, true) ? 1 : 0;
    });
    printf("wrong rule (%s): caught in %ld cases\n", names[w], caught);
    if (!caught) {
      printf("FAILED: the model did not catch %s\n", names[w]);
      ++g_failed;
    }
  }
  printf("%s: %ld cases, %ld failed\n", g_failed ? "FAIL" : "PASS", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
