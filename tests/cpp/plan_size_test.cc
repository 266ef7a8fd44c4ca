// plan_size_test.cc -- the plan sizing rules of csrc/plan_size.h on the CPU (tests/test_plan_size_cpu.py builds and
// runs it; no GPU, no library).  kvsep_crc32c_reserve(count, total) promises that no later call of up to count blocks
// and total bytes allocates -- a captured call that would have to is refused -- so for every piece size such a call can
// pick, the reservation must hold the plan entries the call needs:
//
//   bound      needed(count', total') <= reserved(count, total) for count' <= count, total' <= total, and the same for
//              the SST read check's call (count', total' + count'): it runs len + 1 bytes per block;
//   selection  piece_for is the rule of its comment, restated here: piece_bytes when total / piece_bytes >= want, else
//              the largest of 64 / 32 / 16 KiB that still gives want pieces, else 16 KiB; one size once set explicitly;
//   tightness  the reservation is the maximum of what a call of up to (count, total + count) needs, not a looser bound.
//
// `plan_size_test --rule=parent` runs the bound property against the rule kvsep_crc32c_reserve used before
// (count + total / piece_for(total) + 1: one piece size, the caller's own total) and must FAIL: it lists the grid
// points where a smaller batch, or the SST read check, needs more entries than that rule reserved.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "plan_size.h"

using namespace kvsep;

namespace {
constexpr uint64_t KiB = 1024;

struct Config {
  uint64_t piece_bytes;
  bool piece_auto;
  int num_cus;
};

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The selection rule as piece_for's comment states it.
plan::Piece rule(const Config& c, uint64_t total) {
  if (!c.piece_auto) return {c.piece_bytes, -1};
  const uint64_t want = 2 * uint64_t(c.num_cus) * 8;
  if (total / c.piece_bytes >= want) return {c.piece_bytes, -1};
  for (int k = 2; k >= 0; --k)
    if (total / (16 * KiB << k) >= want) return {16 * KiB << k, k};
  return {16 * KiB, 0};
}

uint64_t needed(const Config& c, uint64_t count, uint64_t total) {
  return count + total / rule(c, total).bytes + 1;
}

bool g_parent_rule = false;

uint64_t reserved(const Config& c, uint64_t count, uint64_t total) {
  if (g_parent_rule) return count + total / rule(c, total).bytes + 1;
  return plan::pieces_reserved(c.piece_bytes, c.piece_auto, c.num_cus, count, total);
}

// Deterministic totals: every threshold want * P (P = 32, 64, 128 KiB and the configured size) and its half, each
// +- {0, 1, 2}; 0 and 1.
std::vector<uint64_t> edge_totals(const Config& c) {
  const uint64_t want = 2 * uint64_t(c.num_cus) * 8;
  std::vector<uint64_t> v = {0, 1};
  for (uint64_t P : {32 * KiB, 64 * KiB, 128 * KiB, c.piece_bytes})
    for (uint64_t t : {want * P, want * P / 2})
      for (int d = -2; d <= 2; ++d)
        if (d >= 0 || t >= uint64_t(-d)) v.push_back(t + uint64_t(int64_t(d)));
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

std::vector<uint64_t> counts() {
  std::vector<uint64_t> v = {0, 1, 0x7fffffffull};
  for (uint64_t P : {16 * KiB, 32 * KiB, 64 * KiB, 128 * KiB}) {
    v.push_back(P - 1);
    v.push_back(P);
    v.push_back(P + 1);
  }
  std::sort(v.begin(), v.end());
  return v;
}

struct Failures {
  uint64_t n = 0, n_batch = 0, n_sst = 0, checked = 0;
  std::set<uint64_t> totals_batch, totals_sst;  // of the current configuration: reservations that were too small
  void report(const Config& c, const char* form, uint64_t count, uint64_t total, uint64_t count2, uint64_t total2,
              uint64_t need, uint64_t have) {
    ++n;
    (std::strcmp(form, "sst") == 0 ? n_sst : n_batch)++;
    (std::strcmp(form, "sst") == 0 ? totals_sst : totals_batch).insert(total);
    if (n <= 12)
      std::printf("BOUND %s cus=%d piece=%" PRIu64 "%s: reserve(%" PRIu64 ", %" PRIu64 ") = %" PRIu64
                  " entries < %" PRIu64 " needed by call(%" PRIu64 ", %" PRIu64 ") at %" PRIu64 "-B pieces\n",
                  form, c.num_cus, c.piece_bytes, c.piece_auto ? " auto" : "", count, total, have, need, count2,
                  total2, rule(c, std::strcmp(form, "sst") == 0 ? total2 + count2 : total2).bytes);
  }
};

void check_bound(const Config& c, const std::vector<uint64_t>& edges, int nrandom, uint64_t seed, Failures& f) {
  const uint64_t want = 2 * uint64_t(c.num_cus) * 8;
  const uint64_t top = 2 * want * std::max<uint64_t>(c.piece_bytes, 128 * KiB) + 5;
  const std::vector<uint64_t> cs = counts();
  std::vector<uint64_t> totals = edges;
  for (int i = 0; i < nrandom; ++i) {
    const uint64_t r = splitmix(seed);
    totals.push_back(i % 4 ? r % top : (r % top) >> (splitmix(seed) % 24));  // a quarter log-spread towards 0
  }
  for (uint64_t total : totals) {
    std::vector<uint64_t> calls;
    for (uint64_t e : edges)
      if (e <= total) calls.push_back(e);
    calls.push_back(total);
    for (int i = 0; i < 12; ++i) calls.push_back(splitmix(seed) % (total + 1));
    for (size_t ci = 0; ci < cs.size(); ++ci) {
      const uint64_t count = cs[ci];
      const uint64_t have = reserved(c, count, total);
      const uint64_t lower[3] = {count, ci ? cs[ci - 1] : 0, count / 2};
      for (uint64_t count2 : lower)
        for (uint64_t total2 : calls) {
          f.checked += 2;
          const uint64_t nb = needed(c, count2, total2);
          if (nb > have) f.report(c, "batch", count, total, count2, total2, nb, have);
          const uint64_t ns = needed(c, count2, total2 + count2);  // the SST read check: len + 1 per block
          if (ns > have) f.report(c, "sst", count, total, count2, total2, ns, have);
        }
    }
  }
}

int check_selection(const Config& c, const std::vector<uint64_t>& edges, uint64_t seed) {
  int bad = 0;
  const uint64_t want = 2 * uint64_t(c.num_cus) * 8;
  const uint64_t top = 2 * want * std::max<uint64_t>(c.piece_bytes, 128 * KiB) + 5;
  std::vector<uint64_t> totals = edges;
  for (int i = 0; i < 4000; ++i) totals.push_back(splitmix(seed) % top);
  for (uint64_t t : totals) {
    const plan::Piece got = plan::piece_for(c.piece_bytes, c.piece_auto, c.num_cus, t), exp = rule(c, t);
    if (got.bytes != exp.bytes || got.table != exp.table) {
      if (++bad <= 10)
        std::printf("SELECT cus=%d piece=%" PRIu64 "%s total=%" PRIu64 ": piece_for %" PRIu64 "/%d, rule %" PRIu64
                    "/%d\n", c.num_cus, c.piece_bytes, c.piece_auto ? " auto" : "", t, got.bytes, got.table,
                    exp.bytes, exp.table);
    }
    if (got.table >= 0 && got.bytes != (kSmallPiece << got.table)) {
      ++bad;
      std::printf("SELECT table %d does not belong to %" PRIu64 "-B pieces\n", got.table, got.bytes);
    }
    if (plan::pieces_needed(got.bytes, 7, t) != 7 + t / got.bytes + 1) {
      ++bad;
      std::printf("NEEDED total=%" PRIu64 "\n", t);
    }
    if (!c.piece_auto && got.bytes != c.piece_bytes) ++bad;  // an explicit size: one P
  }
  return bad;
}

// The reservation is exactly the most any covered call needs.  pieces_needed grows with the total at a fixed piece
// size, so the maximum over all totals <= X is taken at X or just under a threshold: both are among `edges` + X.
int check_tight(const Config& c, const std::vector<uint64_t>& edges, uint64_t seed) {
  int bad = 0;
  const uint64_t want = 2 * uint64_t(c.num_cus) * 8;
  const uint64_t top = 2 * want * std::max<uint64_t>(c.piece_bytes, 128 * KiB) + 5;
  std::vector<uint64_t> totals = edges;
  for (int i = 0; i < 2000; ++i) totals.push_back(splitmix(seed) % top);
  for (uint64_t total : totals)
    for (uint64_t count : counts()) {
      const uint64_t x = total + count;  // what the reservation covers: the SST read check of the caller's numbers
      uint64_t most = needed(c, count, x);
      for (uint64_t e : edges)
        if (e <= x) most = std::max(most, needed(c, count, e));
      const uint64_t have = plan::pieces_reserved(c.piece_bytes, c.piece_auto, c.num_cus, count, total);
      const uint64_t budget = plan::pieces_budget(c.piece_bytes, c.piece_auto, c.num_cus, count, x);
      if (have != most || budget != most) {
        if (++bad <= 10)
          std::printf("TIGHT cus=%d piece=%" PRIu64 "%s: reserve(%" PRIu64 ", %" PRIu64 ") = %" PRIu64
                      ", budget %" PRIu64 ", the most a call needs is %" PRIu64 "\n", c.num_cus, c.piece_bytes,
                      c.piece_auto ? " auto" : "", count, total, have, budget, most);
      }
    }
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--rule=parent") == 0) g_parent_rule = true;
  Failures f;
  int other = 0;
  for (int cus : {1, 64, 256, 304}) {
    const Config configs[] = {{128 * KiB, true, cus},   // the default
                              {128 * KiB, false, cus},  // set explicitly: one P, whatever the batch
                              {64 * KiB, false, cus},  {1024 * KiB, false, cus}, {1 * KiB, false, cus},
                              {1024 * KiB, true, cus}};  // the rule as a pure function of piece_bytes
    for (const Config& c : configs) {
      const std::vector<uint64_t> edges = edge_totals(c);
      check_bound(c, edges, c.piece_auto ? 3000 : 500, 0x5eed0000 + uint64_t(cus), f);
      if (g_parent_rule) {  // which reservations of the deterministic grid were too small
        std::printf("cus=%d piece=%" PRIu64 "%s: reserve(n, total) too small for a smaller batch at total =", cus,
                    c.piece_bytes, c.piece_auto ? " auto" : "");
        for (uint64_t e : edges)
          if (f.totals_batch.count(e)) std::printf(" %" PRIu64, e);
        std::printf(" (+%zu random totals); for the SST read check at %zu of %zu grid totals, %zu totals in all\n",
                    f.totals_batch.size(), std::count_if(edges.begin(), edges.end(), [&](uint64_t e) {
                      return f.totals_sst.count(e) != 0; }), edges.size(), f.totals_sst.size());
        f.totals_batch.clear();
        f.totals_sst.clear();
        continue;
      }
      other += check_selection(c, edges, 0xabc + uint64_t(cus));
      other += check_tight(c, edges, 0xdef + uint64_t(cus));
    }
  }
  std::printf("%s rule: %" PRIu64 " bound checks, %" PRIu64 " failed (%" PRIu64 " batch form, %" PRIu64
              " SST read check); %d selection / tightness failures\n", g_parent_rule ? "parent" : "shipped",
              f.checked, f.n, f.n_batch, f.n_sst, other);
  if (f.n || other) {
    std::printf("FAIL\n");
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
