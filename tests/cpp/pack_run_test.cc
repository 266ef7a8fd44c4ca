// pack_run_test.cc -- the geometry of crc32c_pack_kernel (csrc/pack_run.h) on the CPU, no GPU and no library.
//
// emulate_launch() below is the kernel's control flow (csrc/crc32c_pack.inc) written lane by lane over a memory model:
// every workgroup and wave of both parts of the grid, the lane-parallel descriptor read, the loop over a wave's blocks
// and tiles, the walk of a run in passes of 64 segments, and a span's edge bytes and body granules.  Every index and
// byte decision is a call into pack_run.h, the header the kernel itself includes.  The model checks, per launch:
//   * every destination byte of a block that fits is written exactly once, and no other byte (head, body and tail
//     partition each span; tiles partition a block; each tile has one owner);
//   * the whole destination equals a reference built with memcpy from an independent reading of the contract;
//   * every load is a naturally aligned 16-B granule, or a byte, that holds a byte of a segment of the batch;
//   * seg_off / seg_len are read at indices < nseg only, first for count + 1 elements, dst_off for count.
// Built with -fsanitize=address,undefined by tests/test_pack_run_cpu.py and run as it is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pack_run.h"

using namespace kvsep;

namespace {

constexpr uint64_t kSrcBase = 0x100000, kDstBase = 0x40000000;  // 16-B aligned "addresses"
constexpr uint8_t kCanary = 0xA5;
constexpr uint32_t kWaves = 4;  // kPackThreads / 64

long g_failed = 0, g_cases = 0;
std::string g_case;

void fail(const char* what, uint64_t a = 0, uint64_t b = 0) {
  if (g_failed < 20) printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)a, (unsigned long long)b);
  ++g_failed;
}

struct Batch {
  pack::Frame frame = pack::kPlain;
  std::vector<uint8_t> src;          // the payload, at address kSrcBase
  std::vector<uint64_t> seg_off, seg_len, first, dst_off;
  bool identity = false;             // no first[]: block i is segment i
  std::vector<uint32_t> crc;
  std::vector<uint8_t> types;
  uint64_t count = 0, dst_size = 0, dst_bytes = 0;
  uint32_t wgs = 1024;               // the long part's workgroup budget
};

struct Model {
  const Batch& b;
  std::vector<uint8_t> dst, written, allowed;  // allowed: per source granule
  explicit Model(const Batch& batch) : b(batch), dst(batch.dst_size, kCanary), written(batch.dst_size, 0),
                                       allowed(batch.src.size() / 16 + 2, 0) {
    for (size_t j = 0; j < b.seg_len.size(); ++j)
      if (b.seg_len[j])
        for (uint64_t g = b.seg_off[j] / 16; g < allowed.size() && g <= pack::add_sat(b.seg_off[j], b.seg_len[j] - 1) / 16; ++g)
          allowed[g] = 1;
  }
  uint64_t first_at(uint64_t i) const {
    if (i > b.count) fail("first[] read past count + 1 elements", i);
    return b.first[i];
  }
  uint64_t len_at(uint64_t j) const {
    if (j >= b.seg_len.size()) { fail("a segment index >= nseg was read", j); return 0; }
    return b.seg_len[j];
  }
  uint64_t off_at(uint64_t j) const {
    if (j >= b.seg_off.size()) { fail("a segment index >= nseg was read", j); return 0; }
    return b.seg_off[j];
  }
  void load16(uint64_t addr, uint32_t w[4]) const {
    if (addr & 15) fail("unaligned 16-B load", addr);
    const uint64_t o = addr - kSrcBase;
    if (addr < kSrcBase || o / 16 >= allowed.size() || !allowed[o / 16]) { fail("load of a granule without a segment byte", o); memset(w, 0, 16); return; }
    uint8_t tmp[16] = {0};
    for (int i = 0; i < 16; ++i) if (o + i < b.src.size()) tmp[i] = b.src[o + i];
    memcpy(w, tmp, 16);
  }
  uint8_t load8(uint64_t addr) const {
    const uint64_t o = addr - kSrcBase;
    if (addr < kSrcBase || o >= b.src.size() || !allowed[o / 16]) { fail("byte load outside the segments' granules", o); return 0; }
    return b.src[o];
  }
  void store(uint64_t addr, const void* p, uint64_t n, bool aligned16) {
    if (aligned16 && (addr & 15)) fail("unaligned 16-B store", addr);
    const uint64_t o = addr - kDstBase;
    if (addr < kDstBase || o + n > dst.size()) { fail("store outside the destination buffer", o); return; }
    memcpy(&dst[o], p, n);
    for (uint64_t i = 0; i < n; ++i) ++written[o + i];
  }
};

// pack_span: lanes 0..31 copy the edge bytes, every lane its body granules
void emulate_span(Model& m, uint64_t src, uint64_t dst, uint64_t n) {
  const pack::Span s = pack::split(src, dst, n);
  if (s.body0 - s.dst >= 16 || s.dst + s.n - s.body1 >= 16 || ((s.body1 - s.body0) & 15) || (s.body0 != s.body1 && (s.body0 & 15)))
    fail("split: an edge of 16 bytes or more, or a body that is not whole granules", s.body0, s.body1);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint64_t e = pack::edge_byte(s, lane);
    if (e != ~uint64_t(0)) {
      const uint8_t v = m.load8(src + e);
      m.store(dst + e, &v, 1, false);
    }
  }
  if (s.body0 == s.body1) return;
  const uint64_t iters = pack::body_iters(s);
  for (uint64_t it = 0; it < iters; ++it)
    for (uint32_t lane = 0; lane < 64; ++lane)
      for (uint32_t u = 0; u < pack::kUnroll; ++u) {
        const uint64_t g = pack::body_granule(s, it, u, lane);
        if (!g) continue;
        const uint64_t a = pack::body_src(s, g);
        uint32_t lo[4], hi[4] = {0, 0, 0, 0}, out[4];
        m.load16(a, lo);
        if (s.sh) {
          m.load16(a + 16, hi);
          pack::align16(lo, hi, s.sh, out);
        } else {
          memcpy(out, lo, 16);
        }
        m.store(g, out, 16, true);
      }
}

void emulate_tile(Model& m, pack::Run r, uint64_t total, uint64_t at, uint64_t t) {
  const pack::Range tr = pack::tile_range(total, t);
  uint64_t pos = 0;
  for (uint64_t ps = r.s; ps < r.e && pos < tr.b;) {
    const uint32_t n = pack::pass_segs(ps, r.e);
    uint64_t so[64] = {0}, sl[64] = {0};
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (lane < n) sl[lane] = m.len_at(ps + lane), so[lane] = m.off_at(ps + lane);
    for (uint32_t k = 0; k < n && pos < tr.b; ++k) {
      const pack::Cut c = pack::cut_segment(pos, sl[k], tr);
      if (c.n) emulate_span(m, kSrcBase + so[k] + c.skip, kDstBase + at + c.pos, c.n);
      pos += sl[k];
    }
    ps += n;
  }
}

void emulate_launch(Model& m) {
  const Batch& b = m.b;
  if (!b.count) return;
  const uint64_t nseg = b.seg_len.size();
  const uint64_t per_wg = uint64_t(kWaves) * pack::kShortBlocks;
  const uint64_t short_wgs = (b.count + per_wg - 1) / per_wg;
  const uint32_t team = pack::team_size(b.count, b.wgs);
  const uint64_t grid = short_wgs + pack::chunk_count(b.count) * team;
  for (uint64_t wg = 0; wg < grid; ++wg)
    for (uint32_t wv = 0; wv < kWaves; ++wv) {
      const bool long_part = wg >= short_wgs;
      uint64_t b0;
      uint32_t nb, my = 0, team_waves = 1;
      if (!long_part) {
        b0 = (wg * kWaves + wv) * pack::kShortBlocks, nb = pack::kShortBlocks;
      } else {
        const uint64_t w = wg - short_wgs;
        b0 = (w / team) * pack::kChunkBlocks, nb = pack::kChunkBlocks;
        my = uint32_t(w % team) * kWaves + wv, team_waves = team * kWaves;
      }
      pack::Run r[64];
      uint64_t total[64], d[64];
      bool take[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        take[lane] = false;
        const uint64_t blk = b0 + lane;
        if (!(lane < nb && blk < b.count)) continue;
        r[lane] = b.identity ? pack::clamp_run(blk, blk + 1, nseg) : pack::clamp_run(m.first_at(blk), m.first_at(blk + 1), nseg);
        total[lane] = 0;
        for (uint64_t j = r[lane].s; j < r[lane].e; ++j) total[lane] = pack::add_sat(total[lane], m.len_at(j));
        d[lane] = b.dst_off[blk];
        take[lane] = pack::fits(d[lane], total[lane], b.frame, b.dst_bytes) && (pack::tile_count(total[lane]) > 1) == long_part;
      }
      for (uint32_t src = 0; src < 64; ++src) {
        if (!take[src]) continue;
        const uint64_t tiles = pack::tile_count(total[src]);
        for (uint64_t t = pack::first_tile(src, my, team_waves); t < tiles; t += team_waves) {
          if (!pack::tile_owner(src, t, my, team_waves)) fail("first_tile walks a tile tile_owner gives another wave", src, t);
          if (t == 0) {
            for (uint32_t lane = 0; lane < 64; ++lane) {
              if (b.frame == pack::kVlog && lane < 8) {
                const uint8_t v = pack::vlog_header_byte(b.crc[b0 + src], total[src], lane);
                m.store(kDstBase + d[src] + lane, &v, 1, false);
              }
              if (b.frame == pack::kSst && lane < 5) {
                const uint8_t v = pack::sst_trailer_byte(b.types[b0 + src], b.crc[b0 + src], lane);
                m.store(kDstBase + d[src] + total[src] + lane, &v, 1, false);
              }
            }
          }
          emulate_tile(m, r[src], total[src], d[src] + pack::lead(b.frame), t);
        }
      }
    }
}

// The contract read independently: clamp, sum in 128 bits, memcpy.
void reference(const Batch& b, std::vector<uint8_t>& exp, std::vector<uint8_t>& owned) {
  exp.assign(b.dst_size, kCanary);
  owned.assign(b.dst_size, 0);
  const uint64_t nseg = b.seg_len.size();
  const uint64_t lead = b.frame == pack::kVlog ? 8 : 0, trail = b.frame == pack::kSst ? 5 : 0;
  for (uint64_t i = 0; i < b.count; ++i) {
    uint64_t s = b.identity ? i : b.first[i], e = b.identity ? i + 1 : b.first[i + 1];
    if (s > nseg) s = nseg;
    if (e > nseg) e = nseg;
    if (e < s) e = s;
    unsigned __int128 total = 0;
    for (uint64_t j = s; j < e; ++j) total += b.seg_len[j];
    if ((unsigned __int128)b.dst_off[i] + lead + total + trail > (unsigned __int128)b.dst_bytes) continue;
    uint64_t p = b.dst_off[i];
    if (b.frame == pack::kVlog) {
      const uint32_t h[2] = {b.crc[i], uint32_t(uint64_t(total))};
      memcpy(&exp[p], h, 8);
    }
    p += lead;
    for (uint64_t j = s; j < e; ++j) {
      if (b.seg_len[j]) memcpy(&exp[p], &b.src[b.seg_off[j]], b.seg_len[j]);
      p += b.seg_len[j];
    }
    if (b.frame == pack::kSst) {
      exp[p] = b.types[i];
      memcpy(&exp[p + 1], &b.crc[i], 4);
    }
    for (uint64_t q = b.dst_off[i]; q < p + trail; ++q) ++owned[q];
  }
}

void run_case(const std::string& name, const Batch& b) {
  g_case = name;
  ++g_cases;
  Model m(b);
  emulate_launch(m);
  std::vector<uint8_t> exp, owned;
  reference(b, exp, owned);
  for (uint64_t i = 0; i < b.dst_size; ++i) {
    if (m.written[i] != owned[i]) { fail("a byte written a wrong number of times (offset, times)", i, m.written[i]); break; }
    if (m.dst[i] != exp[i]) { fail("destination differs from memcpy (offset, got)", i, m.dst[i]); break; }
  }
}

std::vector<uint8_t> random_bytes(uint64_t n, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<uint8_t> v(n);
  for (auto& x : v) x = uint8_t(rng());
  return v;
}

// One block of one segment at source alignment sa, destination alignment da, `len` bytes, a 64-byte canary around it.
void one_segment(uint32_t sa, uint32_t da, uint64_t len, const std::vector<uint8_t>& payload) {
  Batch b;
  b.src = payload;
  b.seg_off = {16 + sa};
  b.seg_len = {len};
  b.first = {0, 1};
  b.dst_off = {64 + da};
  b.count = 1;
  b.wgs = 8;  // 32 waves share the tiles (the full budget runs in test_runs)
  b.dst_size = b.dst_bytes = 64 + da + len + 64;
  char name[96];
  snprintf(name, sizeof name, "one segment src %u dst %u len %llu", sa, da, (unsigned long long)len);
  run_case(name, b);
}

void test_alignment_sweep() {
  const uint64_t T = pack::kTile;
  const std::vector<uint8_t> payload = random_bytes(2 * T + 64, 1);
  std::vector<uint64_t> lens;
  for (uint64_t n = 0; n <= 80; ++n) lens.push_back(n);
  for (uint64_t n = T - 17; n <= T + 17; ++n) lens.push_back(n);
  lens.push_back(2 * T - 1), lens.push_back(2 * T + 1);
  for (uint32_t sa = 0; sa < 16; ++sa)
    for (uint32_t da = 0; da < 16; ++da)
      for (uint64_t n : lens) one_segment(sa, da, n, payload);
}

void test_runs() {
  const std::vector<uint8_t> payload = random_bytes(1 << 16, 2);
  std::mt19937 rng(3);
  // blocks back to back, runs of 0 .. 300 segments, zero-length segments at the start, middle and end of a run,
  // segments anywhere (overlapping, shared between blocks through a first[] that steps back)
  for (uint32_t frame = 0; frame < 3; ++frame) {
    Batch b;
    b.frame = pack::Frame(frame);
    b.src = payload;
    const uint32_t runs[] = {0, 1, 2, 8, 65, 300, 3, 64, 63, 129};
    uint64_t at = 77;
    for (uint32_t n : runs) {
      b.first.push_back(b.seg_len.size());
      uint64_t total = 0;
      for (uint32_t k = 0; k < n; ++k) {
        uint64_t len = rng() % 700;
        if (k == 0 || k == n / 2 || k + 1 == n || rng() % 5 == 0) len = 0;
        if (n <= 2) len = 1 + rng() % 40;
        b.seg_len.push_back(len);
        b.seg_off.push_back(rng() % (payload.size() - 700));
        total += len;
      }
      b.dst_off.push_back(at);
      at += pack::lead(b.frame) + total + pack::trail(b.frame);  // no gap: every edge is shared
      b.crc.push_back(rng());
      b.types.push_back(uint8_t(rng()));
    }
    b.first.push_back(b.seg_len.size());
    // two more blocks that reuse earlier segments: first[] steps back
    b.count = b.first.size() - 1;
    b.dst_size = b.dst_bytes = at + 300;
    run_case("runs frame " + std::to_string(frame), b);
    if (frame == 2) {  // the SST form has no first[]: block i is segment i
      Batch s;
      s.frame = pack::kSst, s.identity = true, s.src = payload;
      uint64_t p = 3;
      for (uint32_t i = 0; i < 150; ++i) {
        const uint64_t len = i % 7 == 0 ? 0 : rng() % 5000;
        s.seg_len.push_back(len), s.seg_off.push_back(rng() % (payload.size() - 5000));
        s.dst_off.push_back(p), s.crc.push_back(rng()), s.types.push_back(uint8_t(i));
        p += len + 5;
      }
      s.count = 150, s.dst_size = s.dst_bytes = p + 64;
      run_case("identity runs", s);
    }
  }
  // a long block of many segments cut at odd places, beside short ones: several tiles, several passes, a small team
  for (uint32_t wgs : {1u, 8u, 1024u}) {
    Batch b;
    b.src = random_bytes(600000, 5);
    b.wgs = wgs;
    uint64_t pos = 5;
    for (uint32_t k = 0; k < 200; ++k) {
      const uint64_t len = k % 9 == 0 ? 0 : 1 + rng() % 5000;
      b.seg_off.push_back(pos), b.seg_len.push_back(len);
      pos += len + rng() % 3;
    }
    b.first = {0, 3, 3, 200, 200};
    uint64_t at = 9;
    for (uint32_t i = 0; i < 4; ++i) {
      uint64_t total = 0;
      for (uint64_t j = b.first[i]; j < b.first[i + 1]; ++j) total += b.seg_len[j];
      b.dst_off.push_back(at);
      at += total;
    }
    b.count = 4, b.dst_size = b.dst_bytes = at + 33;
    run_case("long run, budget " + std::to_string(wgs), b);
  }
  // more than one chunk, long blocks in several of them
  {
    Batch b;
    b.src = random_bytes(3 * pack::kTile + 100, 6);
    b.wgs = 16;
    uint64_t at = 1;
    for (uint32_t i = 0; i < 150; ++i) {
      const uint64_t len = i % 50 == 7 ? 2 * pack::kTile + 5 + i : rng() % 300;
      b.seg_off.push_back(rng() % 90), b.seg_len.push_back(len);
      b.first.push_back(i), b.dst_off.push_back(at);
      at += len;
    }
    b.first.push_back(150);
    b.count = 150, b.dst_size = b.dst_bytes = at + 20;
    run_case("three chunks", b);
  }
}

void test_first_garbage() {
  const std::vector<uint8_t> payload = random_bytes(4096, 7);
  const uint64_t big = ~uint64_t(0);
  const std::vector<std::vector<uint64_t>> firsts = {
      {5, 3, 1, 0}, {0, 9, 2, 100}, {big, 0, big, 4}, {2, 2, big, big}, {0, 6, 6, 0}, {7, 1, 6, 3}};
  for (size_t v = 0; v < firsts.size(); ++v) {
    Batch b;
    b.src = payload;
    for (uint32_t j = 0; j < 6; ++j) b.seg_off.push_back(100 * j + j), b.seg_len.push_back(j == 2 ? 0 : 20 + j);
    b.first = firsts[v];
    b.count = 3;
    b.dst_off = {10, 210, 410};
    b.dst_size = b.dst_bytes = 700;
    run_case("first[] garbage " + std::to_string(v), b);
  }
  {  // nseg == 0: every block is empty, nothing is read or written
    Batch b;
    b.src = payload, b.first = {0, 5, big}, b.count = 2, b.dst_off = {3, 3}, b.dst_size = b.dst_bytes = 16;
    run_case("nseg 0", b);
    b.frame = pack::kVlog, b.crc = {0x11223344, 0x55667788}, b.dst_off = {0, 8};
    run_case("nseg 0, vlog headers only", b);
  }
}

void test_fit() {
  const std::vector<uint8_t> payload = random_bytes(4096, 8);
  for (uint32_t frame = 0; frame < 3; ++frame)
    for (int delta = -1; delta <= 1; ++delta) {
      Batch b;
      b.frame = pack::Frame(frame);
      b.src = payload;
      b.seg_off = {3, 500, 1000}, b.seg_len = {100, 37, 200};
      b.first = {0, 1, 2, 3};
      b.crc = {1, 2, 3}, b.types = {4, 5, 6};
      const uint64_t fr = pack::lead(b.frame) + pack::trail(b.frame);
      b.dst_off = {0, 100 + fr, 137 + 2 * fr};
      b.count = 3;
      b.dst_size = 337 + 3 * fr + 64;
      b.dst_bytes = 337 + 3 * fr + delta;  // one short: the last block is not written at all
      run_case("fit frame " + std::to_string(frame) + " delta " + std::to_string(delta), b);
    }
  g_case = "fit predicate";
  const uint64_t big = ~uint64_t(0);
  struct { uint64_t off, len; pack::Frame f; uint64_t bytes; bool ok; } rows[] = {
      {0, 0, pack::kPlain, 0, true},       {1, 0, pack::kPlain, 0, false},      {0, 0, pack::kVlog, 7, false},
      {0, 0, pack::kVlog, 8, true},        {big, 0, pack::kPlain, big, true},   {big, 1, pack::kPlain, big, false},
      {big - 4, 0, pack::kSst, big, false}, {big - 5, 0, pack::kSst, big, true}, {big - 5, 1, pack::kSst, big, false},
      {1, big - 1, pack::kPlain, big, true},   {0, big, pack::kPlain, big, false},   {0, big, pack::kVlog, big, false},
      {big - 7, big - 7, pack::kVlog, big, false}, {10, 5, pack::kPlain, 14, false}, {10, 5, pack::kPlain, 15, true},
  };
  for (auto& r : rows) {
    ++g_cases;
    if (pack::fits(r.off, r.len, r.f, r.bytes) != r.ok) fail("fits() wrong (off, len)", r.off, r.len);
  }
  if (pack::add_sat(big, 1) != big || pack::add_sat(big - 1, 1) != big || pack::add_sat(3, 4) != 7) fail("add_sat");
  // a run whose lengths leave 64 bits fits nowhere and is never walked
  Batch b;
  b.src = payload, b.seg_off = {0, 0}, b.seg_len = {big, 2}, b.first = {0, 2}, b.count = 1, b.dst_off = {0};
  b.dst_size = 64, b.dst_bytes = big;
  Model m(b);
  g_case = "overflowing run";
  ++g_cases;
  emulate_launch(m);
  for (uint8_t w : m.written)
    if (w) { fail("a run longer than 2^64 was written"); break; }
}

void test_tiles() {
  g_case = "tiles";
  const uint64_t T = pack::kTile;
  for (uint64_t total : {uint64_t(0), uint64_t(1), T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 7, ~uint64_t(0)}) {
    ++g_cases;
    const uint64_t n = pack::tile_count(total);
    if ((total <= T) != (n == 1)) fail("tile_count", total, n);
    const uint64_t probe[] = {0, 1, n / 2, n - 1};
    for (uint64_t t : probe) {
      if (t >= n) continue;
      const pack::Range r = pack::tile_range(total, t);
      if (r.a != t * T || r.b < r.a || r.b - r.a > T || (t + 1 == n) != (r.b == total)) fail("tile_range", total, t);
    }
  }
  // every tile of every slot has exactly one owner in a team
  for (uint32_t tw : {1u, 4u, 16u, 4096u})
    for (uint32_t slot : {0u, 1u, 63u})
      for (uint64_t t : {uint64_t(0), uint64_t(5), uint64_t(1) << 40}) {
        uint32_t owners = 0;
        for (uint32_t w = 0; w < tw; ++w) owners += pack::tile_owner(slot, t, w, tw);
        if (owners != 1) fail("tile_owner", tw, t);
      }
  for (uint64_t count : {uint64_t(1), uint64_t(64), uint64_t(65), uint64_t(65536), (uint64_t(1) << 32) - 1}) {
    const uint64_t grid = pack::chunk_count(count) * pack::team_size(count, 1024);
    if (pack::team_size(count, 1024) < pack::kMinTeam || grid >= (uint64_t(1) << 29)) fail("team_size", count, grid);
  }
}

}  // namespace

int main() {
  test_tiles();
  test_fit();
  test_first_garbage();
  test_runs();
  test_alignment_sweep();
  printf("%ld cases, %ld failed\n", g_cases, g_failed);
  puts(g_failed ? "FAIL" : "PASS");
  return g_failed ? 1 : 0;
}
