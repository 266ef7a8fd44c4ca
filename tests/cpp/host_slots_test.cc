// host_slots_test.cc -- the staging-slot grouping rules of csrc/host_slots.h on the CPU (tests/test_host_slots_cpu.py
// builds and runs it; no GPU, no library).  Every host-memory entry point cuts its call into slot jobs by these rules,
// with slot_bytes = 64 MiB and max_blocks = 65,536; here the same header runs with tiny limits (64 / 4, 48 / 3, 16 / 1)
// over every sequence of up to 5 blocks from a small alphabet of lengths (and of up to 4 (off, len) pairs, 5 with
// --deep) and over seeded random sequences of up to 40 blocks:
//
//   partition  the groups and the long blocks cover [0, count) once, in caller order; a block runs alone as a segment
//              chain if and only if len > slot_bytes (len == slot_bytes is grouped); 1 <= blocks of a group <= max_blocks;
//   span       [lo, hi) is the covering range of the group's blocks, hi - lo <= slot_bytes, every block's staged offset
//              off - lo stays inside it whatever order the offsets come in, max_len is the true maximum;
//   gather     staged offsets are 16-B aligned, ascend without overlap, at + len <= slot_bytes, used is the end of the
//              last block, max_len is the true maximum, an empty block has a valid offset;
//   maximal    a group ends only at the end of the call, before a long block, at the block cap, or because the next
//              block would not fit;
//   segments   ceil(n / slot_bytes) of them, each slot_bytes but the last, summing to n;
//   execution  the plan run against a seeded byte buffer: the range (or the pieces) copied into a slot_bytes slot as
//              the plan says, every block checksummed out of the slot (a chain: each segment seeded with the previous
//              result) -- equal to the bytewise CRC-32C of the caller's own bytes.
//
// `host_slots_test --rule=<mutant>` swaps in a deliberately wrong rule written below and must FAIL (exit 1):
//   rel_first     staged offsets taken against the first block's off instead of the group's lo
//   cap_plus1     a block cap of max_blocks + 1
//   no_round      gather packing without the 16-B round-up
//   fit_no_round  gather packing whose fit test ignores the round-up
//   long_ge       len >= slot_bytes treated as long
// The mutants exist only in this CPU program: several of them would write past a staging array in the library.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_slots.h"

using namespace kvsep;

namespace {

enum Rule { kShipped, kRelFirst, kCapPlus1, kNoRound, kFitNoRound, kLongGe };
Rule g_rule = kShipped;

// ---------------------------------------------------------------- the rules under test: the header, or a mutant of it
bool t_is_long(uint64_t len, uint64_t sb) {
  if (g_rule == kLongGe) return len >= sb;
  return slots::is_long(len, sb);
}

slots::SpanGroup t_span_group(const uint64_t* off, const uint64_t* len, uint64_t i, uint64_t count, uint64_t sb,
                              uint64_t mb) {
  if (g_rule == kCapPlus1) return slots::span_group(off, len, i, count, sb, mb + 1);
  if (g_rule == kLongGe) {  // the header's loop, stopping before len >= sb
    slots::SpanGroup g{i + 1, off[i], off[i] + len[i], len[i]};
    while (g.j < count && g.j - i < mb && len[g.j] < sb) {
      const uint64_t nlo = std::min(g.lo, off[g.j]), nhi = std::max(g.hi, off[g.j] + len[g.j]);
      if (nhi - nlo > sb) break;
      g.lo = nlo;
      g.hi = nhi;
      g.max_len = std::max(g.max_len, len[g.j]);
      ++g.j;
    }
    return g;
  }
  return slots::span_group(off, len, i, count, sb, mb);
}

uint64_t t_span_at(const uint64_t* off, uint64_t i, uint64_t k, const slots::SpanGroup& g) {
  if (g_rule == kRelFirst) return off[k] - off[i];
  return slots::span_at(off[k], g);
}

slots::GatherGroup t_gather_group(const uint64_t* len, uint64_t i, uint64_t count, uint64_t sb, uint64_t mb,
                                  uint64_t* at) {
  if (g_rule == kCapPlus1) return slots::gather_group(len, i, count, sb, mb + 1, at);
  if (g_rule == kNoRound || g_rule == kFitNoRound || g_rule == kLongGe) {
    slots::GatherGroup g{i, 0, 0};
    while (g.j < count && g.j - i < mb && !t_is_long(len[g.j], sb)) {
      uint64_t a = (g.used + 15) & ~uint64_t(15);
      if (g_rule == kNoRound) a = g.used;
      if ((g_rule == kFitNoRound ? g.used : a) + len[g.j] > sb) break;
      at[g.j - i] = a;
      g.max_len = std::max(g.max_len, len[g.j]);
      g.used = a + len[g.j];
      ++g.j;
    }
    return g;
  }
  return slots::gather_group(len, i, count, sb, mb, at);
}

// ---------------------------------------------------------------- plumbing
uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint32_t g_table[256];
void init_table() {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1 ? 0x82F63B78u : 0u);  // CRC-32C (Castagnoli), reflected
    g_table[i] = c;
  }
}
// Extend(init, p, n), one byte at a time
uint32_t crc32c(uint32_t init, const uint8_t* p, uint64_t n) {
  uint32_t c = ~init;
  for (uint64_t i = 0; i < n; ++i) c = g_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return ~c;
}

constexpr int kMaxBlocks = 40;

struct Case {
  uint64_t sb, mb;          // the limits
  const uint8_t* buf;       // the caller's bytes
  uint64_t span;            // span form: bytes of the span; gather form: unused
  uint64_t count;
  uint64_t off[kMaxBlocks]; // span form: block offsets; gather form: where each block's pointer points in buf
  uint64_t len[kMaxBlocks];
  uint32_t init[kMaxBlocks];
  uint32_t ref[kMaxBlocks]; // CRC of the caller's own bytes
};

uint64_t g_failures = 0, g_cases = 0, g_groups = 0, g_chains = 0;

void fail(const char* form, const Case& c, const char* what, uint64_t i, uint64_t j) {
  if (++g_failures > 12) return;
  std::printf("FAILED %s slot_bytes=%" PRIu64 " max_blocks=%" PRIu64 " item [%" PRIu64 ", %" PRIu64 "): %s; blocks",
              form, c.sb, c.mb, i, j, what);
  for (uint64_t k = 0; k < c.count; ++k) std::printf(" %" PRIu64 "+%" PRIu64, c.off[k], c.len[k]);
  std::printf("\n");
}

std::vector<uint8_t> g_slot;  // the fake staging slot: exactly slot_bytes, refilled before each job

// A long block: the segment chain, counted, sized and run.
bool check_chain(const char* form, const Case& c, uint64_t i) {
  ++g_chains;
  const uint64_t n = c.len[i], sb = c.sb;
  if (n <= sb) return fail(form, c, "a block of len <= slot_bytes runs as a chain (it must be grouped)", i, i + 1), false;
  const uint64_t cnt = slots::segment_count(n, sb);
  if (cnt != (n + sb - 1) / sb) return fail(form, c, "segment count is not ceil(n / slot_bytes)", i, i + 1), false;
  uint64_t sum = 0;
  uint32_t crc = c.init[i];
  for (uint64_t k = 0; k < cnt; ++k) {
    const slots::Segment s = slots::segment(n, k, sb);
    if (s.at != sum) return fail(form, c, "segments are not back to back", i, i + 1), false;
    if (k + 1 < cnt ? s.bytes != sb : (s.bytes == 0 || s.bytes > sb || s.bytes != n - sum))
      return fail(form, c, "a segment is not slot_bytes (or the last not the remainder)", i, i + 1), false;
    std::memset(g_slot.data(), 0xA5, sb);
    std::memcpy(g_slot.data(), c.buf + c.off[i] + s.at, s.bytes);
    crc = crc32c(crc, g_slot.data(), s.bytes);  // seeded with the previous segment's result
    sum += s.bytes;
  }
  if (sum != n) return fail(form, c, "segments do not sum to n", i, i + 1), false;
  if (crc != c.ref[i]) return fail(form, c, "chained segment CRC differs from the block's CRC", i, i + 1), false;
  return true;
}

// Checks common to both forms for a group [i, j); false: the plan cannot be followed further.
bool check_group_shape(const char* form, const Case& c, uint64_t i, uint64_t j) {
  ++g_groups;
  if (j <= i || j > c.count) return fail(form, c, "group does not advance inside the call", i, j), false;
  if (j - i > c.mb) return fail(form, c, "group has more than max_blocks blocks", i, j), false;
  for (uint64_t k = i; k < j; ++k)
    if (c.len[k] > c.sb) return fail(form, c, "a block over slot_bytes sits in a group", i, j), false;
  return true;
}

void check_span(const Case& c) {
  ++g_cases;
  uint64_t i = 0;
  while (i < c.count) {
    if (t_is_long(c.len[i], c.sb)) {
      if (!check_chain("span", c, i)) return;
      ++i;
      continue;
    }
    const slots::SpanGroup g = t_span_group(c.off, c.len, i, c.count, c.sb, c.mb);
    const uint64_t j = g.j;
    if (!check_group_shape("span", c, i, j)) return;
    uint64_t lo = ~0ull, hi = 0, ml = 0;
    for (uint64_t k = i; k < j; ++k) {
      lo = std::min(lo, c.off[k]);
      hi = std::max(hi, c.off[k] + c.len[k]);
      ml = std::max(ml, c.len[k]);
    }
    if (g.lo != lo || g.hi != hi) return fail("span", c, "[lo, hi) is not the covering range of the group", i, j);
    if (g.hi - g.lo > c.sb) return fail("span", c, "hi - lo > slot_bytes", i, j);
    if (g.hi > c.span) return fail("span", c, "hi past the span", i, j);
    if (g.max_len != ml) return fail("span", c, "max_len is not the group's maximum", i, j);
    if (j < c.count && !(c.len[j] > c.sb || j - i == c.mb ||
                         std::max(hi, c.off[j] + c.len[j]) - std::min(lo, c.off[j]) > c.sb))
      return fail("span", c, "group ended although the next block fits (not maximal)", i, j);
    // execution: the covering range into the slot, every block out of it
    std::memset(g_slot.data(), 0xA5, c.sb);
    std::memcpy(g_slot.data(), c.buf + g.lo, g.hi - g.lo);
    for (uint64_t k = i; k < j; ++k) {
      const uint64_t rel = t_span_at(c.off, i, k, g);
      if (rel > g.hi - g.lo || c.len[k] > g.hi - g.lo - rel)  // a wrapped off - lo lands here too
        return fail("span", c, "a block's staged offset leaves the staged range", i, j);
      if (crc32c(c.init[k], g_slot.data() + rel, c.len[k]) != c.ref[k])
        return fail("span", c, "CRC out of the slot differs from the CRC of the caller's bytes", i, j);
    }
    i = j;
  }
}

void check_gather(const Case& c) {
  ++g_cases;
  uint64_t at[kMaxBlocks + 1];
  uint64_t i = 0;
  while (i < c.count) {
    if (t_is_long(c.len[i], c.sb)) {
      if (!check_chain("gather", c, i)) return;
      ++i;
      continue;
    }
    const slots::GatherGroup g = t_gather_group(c.len, i, c.count, c.sb, c.mb, at);
    const uint64_t j = g.j;
    if (!check_group_shape("gather", c, i, j)) return;
    uint64_t end = 0, ml = 0;
    for (uint64_t k = i; k < j; ++k) {
      const uint64_t a = at[k - i];
      if (a % 16) return fail("gather", c, "a staged offset is not 16-B aligned", i, j);
      if (a < end) return fail("gather", c, "staged offsets do not ascend past the previous block", i, j);
      if (a != ((end + 15) & ~uint64_t(15))) return fail("gather", c, "blocks are not packed back to back", i, j);
      if (a > c.sb || c.len[k] > c.sb - a) return fail("gather", c, "at + len > slot_bytes", i, j);
      end = a + c.len[k];
      ml = std::max(ml, c.len[k]);
    }
    if (g.used != end) return fail("gather", c, "used is not the end of the last block", i, j);
    if (g.max_len != ml) return fail("gather", c, "max_len is not the group's maximum", i, j);
    if (j < c.count && !(c.len[j] > c.sb || j - i == c.mb || ((end + 15) & ~uint64_t(15)) + c.len[j] > c.sb))
      return fail("gather", c, "group ended although the next block fits (not maximal)", i, j);
    // execution: every non-empty piece into the slot first (as the copier pool does), then every block out of it
    std::memset(g_slot.data(), 0xA5, c.sb);
    for (uint64_t k = i; k < j; ++k)
      if (c.len[k]) std::memcpy(g_slot.data() + at[k - i], c.buf + c.off[k], c.len[k]);
    for (uint64_t k = i; k < j; ++k)
      if (crc32c(c.init[k], g_slot.data() + at[k - i], c.len[k]) != c.ref[k])
        return fail("gather", c, "CRC out of the slot differs from the CRC of the caller's bytes", i, j);
    i = j;
  }
}

// ---------------------------------------------------------------- exhaustive: every sequence of up to 5 blocks
constexpr uint64_t kLens[] = {0, 1, 15, 16, 17, 63, 64, 65, 129};
constexpr uint64_t kSpan = 229;  // the block at 100 + 129 ends exactly at the span
constexpr uint64_t kOffs[] = {0, 1, 16, 63, 64, 100, kSpan};
constexpr int kDepth = 5;
constexpr uint32_t kInit[kDepth] = {0, 0xFFFFFFFFu, 0x9E3779B9u, 1, 0x80000000u};

struct Symbol {
  uint64_t off, len;
  uint32_t ref[kDepth];  // by position (the init differs by position)
};

void enumerate(Case& c, const std::vector<Symbol>& syms, bool span_form, int depth, int max_depth) {
  if (g_failures > 12) return;  // a failing rule has shown itself
  if (depth) {
    c.count = uint64_t(depth);
    span_form ? check_span(c) : check_gather(c);
  }
  if (depth == max_depth) return;
  for (const Symbol& s : syms) {
    c.off[depth] = s.off;
    c.len[depth] = s.len;
    c.ref[depth] = s.ref[depth];
    enumerate(c, syms, span_form, depth + 1, max_depth);
  }
}

// Span form, every sequence of lengths with the blocks laid back to back: ascending, and descending from the top of
// a 5 * 129-byte span (lo moves down with every block that joins).
void enumerate_packed(Case& c, bool descending, int depth) {
  if (g_failures > 12) return;
  if (depth) {
    c.count = uint64_t(depth);
    uint64_t p = descending ? c.span : 0;
    for (int k = 0; k < depth; ++k) {
      if (descending) p -= c.len[k];
      c.off[k] = p;
      if (!descending) p += c.len[k];
      c.ref[k] = crc32c(c.init[k], c.buf + c.off[k], c.len[k]);
    }
    check_span(c);
  }
  if (depth == kDepth) return;
  for (uint64_t l : kLens) {
    c.len[depth] = l;
    enumerate_packed(c, descending, depth + 1);
  }
}

void run_exhaustive(const uint8_t* buf, uint64_t sb, uint64_t mb, int pair_depth) {
  Case c{};
  c.sb = sb;
  c.mb = mb;
  c.buf = buf;
  c.span = kSpan;
  std::memcpy(c.init, kInit, sizeof kInit);
  g_slot.assign(sb, 0);
  // span form: every (off, len) of the alphabet that lies inside the span (off == span only with len 0)
  std::vector<Symbol> pairs;
  for (uint64_t o : kOffs)
    for (uint64_t l : kLens)
      if (l <= kSpan - o) pairs.push_back({o, l, {}});
  for (Symbol& s : pairs)
    for (int d = 0; d < kDepth; ++d) s.ref[d] = crc32c(kInit[d], buf + s.off, s.len);
  c.span = kDepth * 129;  // the quick families first: a wrong rule shows itself at once
  enumerate_packed(c, false, 0);
  enumerate_packed(c, true, 0);
  // gather form: every length of the alphabet, each pointer at an odd place of its own in the buffer
  std::vector<Symbol> lens;
  for (size_t k = 0; k < sizeof kLens / sizeof kLens[0]; ++k) lens.push_back({3 + 7 * k, kLens[k], {}});
  for (Symbol& s : lens)
    for (int d = 0; d < kDepth; ++d) s.ref[d] = crc32c(kInit[d], buf + s.off, s.len);
  enumerate(c, lens, false, 0, kDepth);
  c.span = kSpan;
  enumerate(c, pairs, true, 0, pair_depth);
}

// ---------------------------------------------------------------- seeded random sequences of up to 40 blocks
uint64_t random_len(uint64_t& seed, uint64_t sb) {
  const uint64_t r = splitmix(seed);
  switch (r % 8) {
    case 0: return 0;
    case 1: return sb - 1 + (r >> 8) % 3;                 // slot_bytes - 1, slot_bytes, slot_bytes + 1
    case 2: return (r >> 8) % (3 * sb + 3);               // up to 4 segments
    case 3: return kLens[(r >> 8) % 9] % (3 * sb + 3);
    case 4: return 2 * sb - 1 + (r >> 8) % 3;             // the two-segment edge
    default: return (r >> 8) % (sb / 2 + 2);              // short: groups of several blocks
  }
}

void run_random(const uint8_t* buf, uint64_t buf_bytes, uint64_t sb, uint64_t mb, int n, uint64_t seed) {
  g_slot.assign(sb, 0);
  for (int t = 0; t < n; ++t) {
    Case c{};
    c.sb = sb;
    c.mb = mb;
    c.buf = buf;
    c.span = std::min<uint64_t>(buf_bytes, 8 * sb + 37);
    c.count = 1 + splitmix(seed) % kMaxBlocks;
    const uint64_t order = splitmix(seed) % 4;  // 0: random offsets, 1: packed ascending, 2: packed descending,
                                                // 3: all inside a window of slot_bytes + 1 (heavy overlap)
    for (uint64_t k = 0; k < c.count; ++k) {
      c.len[k] = std::min(random_len(seed, sb), c.span);
      c.init[k] = uint32_t(splitmix(seed));
    }
    uint64_t p = 0;
    for (uint64_t k = 0; k < c.count; ++k) {
      const uint64_t room = c.span - c.len[k];
      if (order == 0) {
        c.off[k] = splitmix(seed) % (room + 1);
      } else if (order == 3) {
        c.off[k] = std::min(room, splitmix(seed) % (sb + 2));
      } else {
        if (p > room) p = 0;  // wrap to the start of the span: the offsets then move down inside a group
        c.off[k] = p;
        p += c.len[k] + splitmix(seed) % 3;
      }
      if (splitmix(seed) % 16 == 0 && c.len[k] == 0) c.off[k] = c.span;  // an empty block at the very end
    }
    if (order == 2) {
      std::reverse(c.off, c.off + c.count);
      std::reverse(c.len, c.len + c.count);
    }
    for (uint64_t k = 0; k < c.count; ++k) c.ref[k] = crc32c(c.init[k], buf + c.off[k], c.len[k]);
    check_span(c);
    check_gather(c);  // the same blocks through their pointers buf + off
  }
}

}  // namespace

int main(int argc, char** argv) {
  // Sequences of (off, len) pairs: the alphabet has 55 pairs inside the span, so up to 4 blocks (9.3 million sequences
  // per pair of limits) by default and up to 5 (1.5e9 in all, a quarter of an hour) with --deep.  Sequences of lengths,
  // for the gather form and for the span form's packed layouts, always run up to 5 blocks.
  int pair_depth = 4;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (std::strcmp(a, "--rule=rel_first") == 0) g_rule = kRelFirst;
    else if (std::strcmp(a, "--rule=cap_plus1") == 0) g_rule = kCapPlus1;
    else if (std::strcmp(a, "--rule=no_round") == 0) g_rule = kNoRound;
    else if (std::strcmp(a, "--rule=fit_no_round") == 0) g_rule = kFitNoRound;
    else if (std::strcmp(a, "--rule=long_ge") == 0) g_rule = kLongGe;
    else if (std::strcmp(a, "--deep") == 0) pair_depth = kDepth;
    else if (std::strcmp(a, "--rule=shipped") != 0) {
      std::printf("unknown argument %s\n", a);
      return 2;
    }
  }
  static_assert(kSlotBytes == (64ull << 20) && kSlotBlocks == 65536, "the limits the GPU tests are written for");
  init_table();
  std::vector<uint8_t> buf(1 << 16);
  uint64_t seed = 0x5107b17e5ull;
  for (uint8_t& b : buf) b = uint8_t(splitmix(seed) >> 11);

  const uint64_t limits[][2] = {{64, 4}, {48, 3}, {16, 1}};
  for (const auto& l : limits) run_exhaustive(buf.data(), l[0], l[1], pair_depth);
  const uint64_t exhaustive = g_cases;
  const uint64_t more[][2] = {{64, 4}, {48, 3}, {16, 1}, {256, 8}, {1024, 40}, {4096, 2}};
  for (const auto& l : more) run_random(buf.data(), buf.size(), l[0], l[1], 1500, 0xabcd0000 + l[0] * 131 + l[1]);

  const char* names[] = {"shipped", "rel_first", "cap_plus1", "no_round", "fit_no_round", "long_ge"};
  std::printf("%s rule: %" PRIu64 " exhaustive and %" PRIu64 " random sequences, %" PRIu64 " groups, %" PRIu64
              " segment chains, %" PRIu64 " failed\n", names[g_rule], exhaustive, g_cases - exhaustive, g_groups,
              g_chains, g_failures);
  if (g_failures) {
    std::printf("FAIL\n");
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
