// concat_run_test.cc -- the run arithmetic of crc32c_concat_kernel (csrc/concat_run.h) on the CPU
// (tests/test_concat_run_cpu.py builds and runs it; no GPU, no library).  The kernel takes every index decision from
// that header; here the same header drives an emulation of the kernel's launch -- workgroups of 4 wavefronts, 16 blocks
// per wavefront, short runs folded by their lane, long runs by 64 lanes in passes, one contiguous chunk per lane, then
// the ordered 6-level lane tree -- over arrays whose every access is recorded, and the result is compared with a plain
// serial fold written out below:
//
//   exhaustive  every first[] of count + 1 values from {0 .. nseg + 1, 2^64 - 1} for count <= 4, nseg <= 5 -- decreasing
//               values and values above nseg included;
//   long        the same over {0, 1, 38, 40, 41, 2^64 - 1} for count <= 3, nseg = 40, where runs of 38 .. 40 segments
//               take the wavefront path;
//   random      seeded batches of up to 40 blocks with runs from 0 to three passes (3,072 segments), segment lengths
//               from 0 to 2^64 - 1, sometimes with a malformed first[];
//   each case   out[i] equals the serial fold for every i < count; seg_crc / seg_len are read at indices < nseg only,
//               first at indices <= count, init and out at indices < count, and out is written exactly once per block.
//
// `concat_run_test --rule=<mutant>` swaps in a deliberately wrong rule written below and must FAIL (exit 1):
//   swap         the tree joins (right, left) instead of (left, right)
//   no_clamp     first[] used as it comes
//   chunk_floor  floor(n / 64) segments per lane instead of ceil
// The mutants exist only in this CPU program: no_clamp would read outside the arrays in the library.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "concat_run.h"
#include "gf2.h"

using namespace kvsep;

namespace {

enum Rule { kShipped, kSwap, kNoClamp, kChunkFloor };
Rule g_rule = kShipped;

struct Mul {
  uint32_t operator()(uint32_t a, uint32_t b) const { return gf2::mulmod(a, b); }
};

// ---------------------------------------------------------------- the rules under test: the header, or a mutant of it
concat::Run t_clamp_run(uint64_t f0, uint64_t f1, uint64_t nseg) {
  if (g_rule == kNoClamp) return {f0, f1 < f0 ? f0 : f1};
  return concat::clamp_run(f0, f1, nseg);
}
uint64_t t_lane_chunk(uint64_t n) {
  if (g_rule == kChunkFloor) return n / concat::kWaveLanes;
  return concat::lane_chunk(n);
}
concat::Pair t_join(const concat::Pair& left, const concat::Pair& right) {
  if (g_rule == kSwap) return concat::compose(right, left, Mul());
  return concat::compose(left, right, Mul());
}

// ---------------------------------------------------------------- a batch whose every access is recorded
struct Batch {
  std::vector<uint32_t> seg_crc, seg_mul;  // seg_mul[j] = X(seg_len[j]): what the kernel builds from seg_len[j]
  std::vector<uint64_t> first;
  std::vector<uint32_t> init;
  bool with_init = true;
  uint64_t count = 0, nseg = 0;
  // the record
  std::vector<uint32_t> out, writes;
  uint64_t bad_seg = 0, bad_first = 0, bad_block = 0;

  concat::Pair seg(uint64_t j) {
    if (j >= nseg) {  // only counted, never made; the emulation stops its loops at the first one
      ++bad_seg;
      return concat::identity();
    }
    return {seg_mul[j], seg_crc[j]};
  }
  uint64_t first_at(uint64_t i) {
    if (i > count) {
      ++bad_first;
      return 0;
    }
    return first[i];
  }
  uint32_t init_at(uint64_t i) {
    if (i >= count) {
      ++bad_block;
      return 0;
    }
    return with_init ? init[i] : 0u;
  }
  void write(uint64_t i, uint32_t v) {
    if (i >= count) {
      ++bad_block;
      return;
    }
    out[i] = v;
    ++writes[i];
  }
};

// The plain fold: block i is segments [min(first[i], nseg), min(first[i + 1], nseg)), empty when that ends before it
// starts; acc <- acc * X(seg_len[j]) ^ seg_crc[j].
uint32_t plain(const Batch& b, uint64_t i) {
  uint64_t s = b.first[i] < b.nseg ? b.first[i] : b.nseg;
  uint64_t e = b.first[i + 1] < b.nseg ? b.first[i + 1] : b.nseg;
  uint32_t acc = b.with_init ? b.init[i] : 0u;
  for (uint64_t j = s; j < e; ++j) acc = gf2::mulmod(acc, b.seg_mul[j]) ^ b.seg_crc[j];
  return acc;
}

// ---------------------------------------------------------------- the kernel's launch, lane by lane
void wave(Batch& b, uint64_t w) {
  concat::Run r[concat::kWaveLanes];
  uint32_t acc[concat::kWaveLanes];
  bool is_long[concat::kWaveLanes];
  for (uint32_t lane = 0; lane < concat::kWaveLanes; ++lane) {
    const uint64_t blk = w * concat::kWaveBlocks + lane;
    const bool own = lane < concat::kWaveBlocks && blk < b.count;
    r[lane] = {0, 0};
    acc[lane] = 0;
    if (own) {
      r[lane] = t_clamp_run(b.first_at(blk), b.first_at(blk + 1), b.nseg);
      acc[lane] = b.init_at(blk);
    }
    is_long[lane] = own && !concat::is_short(r[lane]);
    if (own && !is_long[lane]) {
      for (uint64_t j = r[lane].s; j < r[lane].e && !b.bad_seg; ++j) {
        const concat::Pair sg = b.seg(j);
        acc[lane] = gf2::mulmod(acc[lane], sg.m) ^ sg.v;
      }
      b.write(blk, acc[lane]);
    }
  }
  for (uint32_t src = 0; src < concat::kWaveLanes; ++src) {
    if (!is_long[src]) continue;
    const uint64_t e = r[src].e;
    uint32_t run_acc = acc[src];
    for (uint64_t ps = r[src].s; ps < e && !b.bad_seg;) {
      const uint64_t pe = concat::pass_end(ps, e);
      const uint64_t chunk = t_lane_chunk(pe - ps);
      concat::Pair p[concat::kWaveLanes];
      for (uint32_t lane = 0; lane < concat::kWaveLanes; ++lane) {
        const concat::Run mine = concat::lane_range(ps, pe, chunk, lane);
        p[lane] = concat::identity();
        for (uint64_t j = mine.s; j < mine.e; ++j) p[lane] = concat::compose(p[lane], b.seg(j), Mul());
      }
      for (int level = 0; level < concat::kTreeLevels; ++level) {
        concat::Pair q[concat::kWaveLanes];
        for (uint32_t lane = 0; lane < concat::kWaveLanes; ++lane)
          q[lane] = concat::tree_joins(lane, level) ? t_join(p[concat::tree_partner(lane, level)], p[lane]) : p[lane];
        std::memcpy(p, q, sizeof p);
      }
      run_acc = gf2::mulmod(run_acc, p[63].m) ^ p[63].v;
      ps = pe;
    }
    b.write(w * concat::kWaveBlocks + src, run_acc);
  }
}

void launch(Batch& b) {
  b.out.assign(b.count, 0xdeadbeefu);
  b.writes.assign(b.count, 0);
  b.bad_seg = b.bad_first = b.bad_block = 0;
  if (!b.count) return;  // no launch
  constexpr uint64_t kWaves = 4, kPerWg = kWaves * concat::kWaveBlocks;
  const uint64_t grid = (b.count + kPerWg - 1) / kPerWg;
  for (uint64_t wg = 0; wg < grid; ++wg)
    for (uint64_t w = 0; w < kWaves; ++w) wave(b, wg * kWaves + w);
}

// ---------------------------------------------------------------- checking
uint64_t g_cases = 0, g_failed = 0;

void check(Batch& b, const char* family) {
  ++g_cases;
  launch(b);
  const char* why = nullptr;
  uint64_t at = 0;
  if (b.bad_seg) why = "a segment index >= nseg was read";
  else if (b.bad_first) why = "first[] was read past count";
  else if (b.bad_block) why = "init / out touched at an index >= count";
  for (uint64_t i = 0; i < b.count && !why; ++i) {
    at = i;
    if (b.writes[i] != 1) why = "out[i] not written exactly once";
    else if (b.out[i] != plain(b, i)) why = "out[i] differs from the serial fold";
  }
  if (!why) return;
  if (++g_failed <= 5) {
    std::printf("FAILED %s: %s (block %" PRIu64 ", count %" PRIu64 ", nseg %" PRIu64 ", first", family, why, at,
                b.count, b.nseg);
    for (uint64_t k = 0; k <= b.count && k < 8; ++k) std::printf(" %" PRIu64, b.first[k]);
    std::printf(")\n");
  }
}

uint64_t g_state = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const uint64_t kLens[] = {0, 1, 3, 4096, (1ull << 32) + 77, (1ull << 61) - 1, 1ull << 61, (1ull << 61) + 1,
                          1ull << 63, ~0ull};

void fill_segments(Batch& b, uint64_t nseg) {
  b.nseg = nseg;
  b.seg_crc.resize(nseg);
  b.seg_mul.resize(nseg);
  for (uint64_t j = 0; j < nseg; ++j) {
    const uint64_t pick = rnd() % 12;
    b.seg_crc[j] = uint32_t(rnd());
    b.seg_mul[j] = gf2::xpow8(pick < 10 ? kLens[pick] : rnd());
  }
}

void set_count(Batch& b, uint64_t count) {
  b.count = count;
  b.first.assign(count + 1, 0);
  b.init.resize(count);
  for (auto& v : b.init) v = uint32_t(rnd());
}

// every first[] of count + 1 values from the alphabet
void every_first(Batch& b, const std::vector<uint64_t>& alphabet, const char* family) {
  std::vector<size_t> digit(b.count + 1, 0);
  for (;;) {
    for (uint64_t k = 0; k <= b.count; ++k) b.first[k] = alphabet[digit[k]];
    b.with_init = (g_cases & 1) != 0;
    check(b, family);
    size_t k = 0;
    while (k <= b.count && ++digit[k] == alphabet.size()) digit[k++] = 0;
    if (k > b.count) break;
  }
}

// X(n) itself, where 8n fits: x^8 multiplied n times, and X(a) X(b) = X(a + b) around the top three bits.
void check_xpow8() {
  ++g_cases;
  const uint32_t x8 = gf2::xpow(8);
  uint32_t p = concat::kOne;
  bool ok = gf2::xpow(0) == concat::kOne && gf2::xpow(1) == 0x40000000u;
  for (uint64_t n = 0; n < 300 && ok; ++n, p = gf2::mulmod(p, x8)) ok = gf2::xpow8(n) == p;
  const uint64_t big[] = {(1ull << 61) - 1, 1ull << 61, (1ull << 62) + 12345, (1ull << 63) - 1};
  for (uint64_t a : big)
    for (uint64_t d : {1ull, 77ull, 1ull << 33, 1ull << 61})
      ok = ok && gf2::mulmod(gf2::xpow8(a), gf2::xpow8(d)) == gf2::xpow8(a + d);  // a + d < 2^64
  ok = ok && gf2::combine(0x12345678u, 0u, 0) == 0x12345678u;
  if (!ok) {
    ++g_failed;
    std::printf("FAILED xpow8: X(n) differs from repeated multiplication\n");
  }
}

}  // namespace

int main(int argc, char** argv) {
  const char* name = "shipped";
  for (int i = 1; i < argc; ++i) {
    if (std::strncmp(argv[i], "--rule=", 7) != 0) return 2;
    name = argv[i] + 7;
    if (!std::strcmp(name, "swap")) g_rule = kSwap;
    else if (!std::strcmp(name, "no_clamp")) g_rule = kNoClamp;
    else if (!std::strcmp(name, "chunk_floor")) g_rule = kChunkFloor;
    else return 2;
  }
  check_xpow8();
  Batch b;
  for (uint64_t nseg = 0; nseg <= 5; ++nseg) {
    fill_segments(b, nseg);
    std::vector<uint64_t> alphabet;
    for (uint64_t v = 0; v <= nseg + 1; ++v) alphabet.push_back(v);
    alphabet.push_back(~0ull);
    for (uint64_t count = 0; count <= 4; ++count) {
      set_count(b, count);
      every_first(b, alphabet, "exhaustive");
    }
  }
  fill_segments(b, 40);
  for (uint64_t count = 1; count <= 3; ++count) {
    set_count(b, count);
    every_first(b, {0, 1, 38, 40, 41, ~0ull}, "long");
  }
  for (int round = 0; round < 60; ++round) {
    const uint64_t count = 1 + rnd() % 40;
    std::vector<uint64_t> runs(count);
    uint64_t nseg = 0;
    for (auto& n : runs) {
      const uint64_t kind = rnd() % 8;
      n = kind == 0   ? 0
          : kind == 1 ? concat::kShortMax - 1 + rnd() % 3                  // around the short / long threshold
          : kind == 2 ? concat::kPassSegs - 1 + rnd() % 3                  // around one pass
          : kind == 3 ? rnd() % (3 * concat::kPassSegs + 1)                // up to three passes
          : kind == 4 ? 63 + rnd() % 3
                      : rnd() % 70;
      nseg += n;
    }
    fill_segments(b, nseg + rnd() % 3);  // sometimes segments no block uses
    set_count(b, count);
    for (uint64_t i = 0; i < count; ++i) b.first[i + 1] = b.first[i] + runs[i];
    if (round % 4 == 3) {  // malformed: a few entries moved anywhere
      for (int k = 0; k < 3; ++k) {
        const uint64_t kind = rnd() % 3;
        b.first[rnd() % (count + 1)] = kind == 0 ? ~0ull - rnd() % 3 : kind == 1 ? nseg + rnd() % 5 : rnd() % (nseg + 1);
      }
    }
    b.with_init = (round & 1) != 0;
    check(b, "random");
  }
  std::printf("%s rule: %" PRIu64 " cases, %" PRIu64 " failed\n", name, g_cases, g_failed);
  std::printf(g_failed ? "FAIL\n" : "PASS\n");
  return g_failed ? 1 : 0;
}
