// route_test.cc -- the routing rule of csrc/route.h on the CPU (tests/test_route_cpu.py builds and runs it; no GPU, no
// library).  route::decide() replaced five functions of crc32c_device.hip that took the context -- ragged_batch,
// claim16_route, narrow_form, use_narrow, route_batch -- and three callers that each combined their answers in their own
// way.  Namespace `parent` below carries those five functions as they stood in the commit before route.h (the one edit:
// `c` is a plain struct here), and answer() combines them the way that commit's launch_batch_body,
// kvsep_crc32c_plan_query and kvsep_crc32c_kernel_name did.  decide() must equal that in every field -- planned, piece
// bytes, table, schedule, wide / narrow, form, hint, workgroup, combine grid, plan entries, kernel name -- on a grid of
// every threshold +- 1 and on 10^6 random points.  The program prints how many points reached each form and fails if a
// form or a schedule was reached by none.
//
// `route_test --candidate=claim-bound | ragged-order | coop-hint` compares the parent rule with a deliberately wrong
// one in decide()'s place (the claim kernel's upper bound off by one; ragged tested after claim16; the coop hint left
// unclamped) and must FAIL: the grid sees each of them.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "route.h"

namespace parent {
namespace plan = kvsep::plan;

// the constants the five functions read, as that commit had them
constexpr int kWgThreads = 512;
constexpr uint64_t kNarrowMax = 32 * 1024;
constexpr uint64_t kCoopMaxLen = 4096;
constexpr uint32_t kCombineMaxGrid = 2048;

struct DevTables {
  uint32_t zpiece[4][256];
  uint32_t zsmall[3][4][256];
};

struct kvsep_crc32c_ctx {
  int num_cus;
  DevTables* d_tabs;
  uint64_t piece_bytes;
  bool piece_auto;
  int dynamic;
  int kernel;
};

// the shipped library's hook (crc32c_diag.inc): no override
inline int diag_use_narrow(const kvsep_crc32c_ctx*) { return -1; }

// ---- verbatim from crc32c_device.hip (comments shortened) ----
bool ragged_batch(uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  return count != 0 && total_bytes != 0 && 4 * max_len > 5 * (total_bytes / count);
}

bool claim16_route(uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  const uint64_t bytes = total_bytes ? total_bytes : count * max_len;
  return max_len >= 8 * 1024 && max_len <= 12 * 1024 && count >= 4096 && bytes <= (512ull << 20);
}

int narrow_form(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  if (c->kernel == 3) return 6;
  if (c->kernel == 4) return 9;
  if (c->kernel == 5) return 20;
  if (c->kernel == 6) return 10;
  if (c->kernel == 7) return 11;
  if (c->kernel == 8) return 12;
  if (ragged_batch(count, total_bytes, max_len)) return 20;
  if (claim16_route(count, total_bytes, max_len)) return 11;
  if (max_len <= 8 * 1024 && count >= (1u << 15) && count <= (max_len <= 4 * 1024 ? 3u << 17 : 1u << 16)) return 10;
  const bool eight_waves = max_len <= 8 * 1024 ? count >= (1u << 17) : count >= (1u << 15);
  return eight_waves ? 9 : 6;
}

bool use_narrow(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  if (max_len == 0 || max_len > 2 * kNarrowMax) return false;
  if (c->kernel == 1) return false;
  if (c->kernel >= 2) return true;
  const int d = diag_use_narrow(c);  // KVSEP_DIAG build only: -1 (no override) in the shipped library
  if (d >= 0) return d != 0;
  if (claim16_route(count, total_bytes, max_len) && !ragged_batch(count, total_bytes, max_len)) return true;
  const uint64_t cus = uint64_t(c->num_cus);
  return (max_len <= 8 * 1024 && count >= 32 * cus) || (max_len <= 16 * 1024 && count >= 64 * cus) ||
         (max_len <= kNarrowMax && count >= 128 * cus);
}

struct Route {
  bool planned;
  uint64_t piece_bytes;
  const uint32_t* zpiece;
  bool dyn;
};

Route route_batch(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  Route r;
  r.planned = !(max_len != 0 && max_len <= c->piece_bytes);
  r.piece_bytes = c->piece_bytes;
  r.zpiece = &c->d_tabs->zpiece[0][0];
  if (r.planned) {
    const plan::Piece p = plan::piece_for(c->piece_bytes, c->piece_auto, c->num_cus, total_bytes);
    r.piece_bytes = p.bytes;
    if (p.table >= 0) r.zpiece = &c->d_tabs->zsmall[p.table][0][0];
  }
  const uint64_t est_items = r.planned ? count + total_bytes / r.piece_bytes : count;
  const uint64_t nwaves_est = uint64_t(c->num_cus) * (kWgThreads / 64);
  r.dyn = c->dynamic < 0 ? (r.planned && est_items >= 8 * nwaves_est) : c->dynamic == 1;
  return r;
}
// ---- end of the verbatim part ----
}  // namespace parent

namespace {
using kvsep::route::Form;
using parent::kvsep_crc32c_ctx;
constexpr uint64_t KiB = 1024, MiB = 1024 * 1024;

// Everything a caller of the routing took from it.
struct Answer {
  bool planned;
  uint64_t piece_bytes;
  int table;
  bool dyn;
  bool narrow;
  int form;  // 0 wide, else the narrow form's number
  uint64_t hint;
  unsigned threads;
  unsigned combine_grid;
  uint64_t pieces_needed;
  const char* name;
};

// The deliberately wrong rules: the parent's, but for one line.
using NarrowForm = int (*)(const kvsep_crc32c_ctx*, uint64_t, uint64_t, uint64_t);

int narrow_form_claim_bound(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  // `count <= bound` read as `count <= bound + 1`
  if (c->kernel < 3 && !parent::ragged_batch(count, total_bytes, max_len) &&
      !parent::claim16_route(count, total_bytes, max_len) && max_len <= 8 * KiB &&
      count == (max_len <= 4 * KiB ? 3u << 17 : 1u << 16) + 1)
    return 10;
  return parent::narrow_form(c, count, total_bytes, max_len);
}

int narrow_form_ragged_order(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  if (c->kernel < 3 && parent::claim16_route(count, total_bytes, max_len)) return 11;  // before the ragged test
  return parent::narrow_form(c, count, total_bytes, max_len);
}

// The parent's three callers.  launch_batch_body: the kernel, the hint it passed (clamped for form 12), the workgroup of
// each case of its switch, the combine grid its slots reduce counted (grid + (planned ? cgrid : 0)).
// kvsep_crc32c_plan_query: piece bytes, plan entries, schedule.  kvsep_crc32c_kernel_name: its own `planned` and chain.
Answer answer(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len,
              NarrowForm narrow_form = parent::narrow_form, bool clamp = true) {
  Answer a;
  const parent::Route r = parent::route_batch(c, count, total_bytes, max_len);
  a.planned = r.planned;
  a.piece_bytes = r.piece_bytes;
  a.table = -1;
  for (int k = 0; k < 3; ++k)
    if (r.zpiece == &c->d_tabs->zsmall[k][0][0]) a.table = k;
  a.dyn = r.dyn;
  a.pieces_needed = r.planned ? kvsep::plan::pieces_needed(r.piece_bytes, count, total_bytes) : 0;
  a.narrow = !r.planned && parent::use_narrow(c, count, total_bytes, max_len);
  a.form = 0;
  a.hint = 0;
  a.threads = parent::kWgThreads;
  if (a.narrow) {
    const int nv = narrow_form(c, count, total_bytes, max_len);
    a.form = nv;
    a.hint = max_len;
    if (clamp && nv == 12 && a.hint > parent::kCoopMaxLen) a.hint = parent::kCoopMaxLen;
    a.threads = nv == 9 || nv == 10 || nv == 11 || nv == 12 ? 512 : 1024;  // (20 and the default case: 1024)
  }
  const unsigned cgrid = unsigned(std::min<uint64_t>((count + 255) / 256, parent::kCombineMaxGrid));
  a.combine_grid = r.planned ? cgrid : 0u;
  const bool planned = !(max_len != 0 && max_len <= c->piece_bytes);
  if (planned || !parent::use_narrow(c, count, total_bytes, max_len)) {
    a.name = "crc32c_pieces_kernel";
  } else {
    const int nf = narrow_form(c, count, total_bytes, max_len);
    a.name = nf == 20 ? "crc32c_narrow_sorted_kernel"
             : nf == 10 || nf == 11 ? "crc32c_narrow_claim_kernel"
             : nf == 12             ? "crc32c_narrow_coop_kernel"
                                    : "crc32c_narrow_kernel";
  }
  return a;
}

Answer decided(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  const kvsep::route::Settings s{c->num_cus, c->piece_bytes, c->piece_auto, c->dynamic, kvsep::route::Kernel(c->kernel)};
  const kvsep::route::Route r = kvsep::route::decide(s, count, total_bytes, max_len);
  return Answer{r.planned, r.piece.bytes, r.piece.table, r.dyn, r.form != Form::Wide, int(r.form), r.hint, r.threads,
                r.combine_grid, r.pieces_needed, kvsep::route::kernel_name(r.form)};
}

enum Candidate { kDecide, kClaimBound, kRaggedOrder, kCoopHint };
Candidate g_candidate = kDecide;

Answer candidate(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  switch (g_candidate) {
    case kClaimBound: return answer(c, count, total_bytes, max_len, narrow_form_claim_bound);
    case kRaggedOrder: return answer(c, count, total_bytes, max_len, narrow_form_ragged_order);
    case kCoopHint: return answer(c, count, total_bytes, max_len, parent::narrow_form, false);
    default: return decided(c, count, total_bytes, max_len);
  }
}

uint64_t g_checked = 0, g_failed = 0;
std::map<int, uint64_t> g_forms;
uint64_t g_sched[2] = {0, 0}, g_planned = 0;

void check(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  const Answer p = answer(c, count, total_bytes, max_len), d = candidate(c, count, total_bytes, max_len);
  ++g_checked;
  ++g_forms[p.form];
  ++g_sched[p.dyn ? 1 : 0];
  g_planned += p.planned ? 1 : 0;
  const bool same = p.planned == d.planned && p.piece_bytes == d.piece_bytes && p.table == d.table && p.dyn == d.dyn &&
                    p.narrow == d.narrow && p.form == d.form && p.hint == d.hint && p.threads == d.threads &&
                    p.combine_grid == d.combine_grid && p.pieces_needed == d.pieces_needed &&
                    std::strcmp(p.name, d.name) == 0;
  if (same) return;
  if (++g_failed > 10) return;
  std::printf("DIFF cus=%d kernel=%d dynamic=%d piece=%" PRIu64 "%s count=%" PRIu64 " total=%" PRIu64 " max_len=%" PRIu64
              "\n", c->num_cus, c->kernel, c->dynamic, c->piece_bytes, c->piece_auto ? " auto" : "", count, total_bytes,
              max_len);
  const Answer* both[2] = {&p, &d};
  for (int i = 0; i < 2; ++i) {
    const Answer& a = *both[i];
    std::printf("  %-9s planned=%d piece=%" PRIu64 "/%d dyn=%d narrow=%d form=%d hint=%" PRIu64 " threads=%u cgrid=%u "
                "pieces=%" PRIu64 " %s\n", i ? "candidate" : "parent", a.planned, a.piece_bytes, a.table, a.dyn,
                a.narrow, a.form, a.hint, a.threads, a.combine_grid, a.pieces_needed, a.name);
  }
}

void around(std::vector<uint64_t>& v, uint64_t t) {
  for (uint64_t x : {t - 1, t, t + 1}) v.push_back(x);
}

void dedupe(std::vector<uint64_t>& v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The totals of one (count, max_len): unknown; uniform; the means on either side of the ragged rule
// 4 max_len > 5 (total / count); 512 MiB (claim16) and the piece-size thresholds want_pieces * {32, 64, 128 KiB}, +- 1.
std::vector<uint64_t> totals(int cus, uint64_t count, uint64_t max_len) {
  std::vector<uint64_t> v = {0, count * max_len};
  const uint64_t even = (4 * max_len + 4) / 5;  // the smallest mean that is not ragged
  v.push_back(count * even);
  if (count != 0 && even != 0) v.push_back(count * even - 1);  // a mean of even - 1: ragged
  around(v, 512 * MiB);
  for (uint64_t P : {32 * KiB, 64 * KiB, 128 * KiB}) around(v, kvsep::plan::want_pieces(cus) * P);
  dedupe(v);
  return v;
}

void grid() {
  static parent::DevTables tabs;
  const struct { uint64_t bytes; bool is_auto; } pieces[] = {{128 * KiB, true}, {128 * KiB, false}, {1 * KiB, false},
                                                            {1 * MiB, false}};
  for (int cus : {1, 8, 64, 256, 304})
    for (int kernel = 0; kernel <= 8; ++kernel)
      for (int dynamic = -1; dynamic <= 1; ++dynamic)
        for (const auto& pc : pieces) {
          const kvsep_crc32c_ctx c{cus, &tabs, pc.bytes, pc.is_auto, dynamic, kernel};
          std::vector<uint64_t> lens = {0, 1}, counts = {0, 1, 0xffffffffull};
          for (uint64_t t : {4 * KiB, 8 * KiB, 12 * KiB, 16 * KiB, 32 * KiB, 64 * KiB, pc.bytes}) around(lens, t);
          const uint64_t u = uint64_t(cus);
          for (uint64_t t : {uint64_t(4096), uint64_t(1) << 15, uint64_t(1) << 16, uint64_t(1) << 17, uint64_t(3) << 17,
                             32 * u, 64 * u, 128 * u, 8 * u * 8})
            around(counts, t);
          dedupe(lens);
          dedupe(counts);
          for (uint64_t max_len : lens)
            for (uint64_t count : counts)
              for (uint64_t total : totals(cus, count, max_len)) check(&c, count, total, max_len);
        }
}

void random_points(uint64_t n, uint64_t seed) {
  static parent::DevTables tabs;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t a = splitmix(seed), b = splitmix(seed), d = splitmix(seed), e = splitmix(seed);
    kvsep_crc32c_ctx c;
    c.num_cus = 1 + int(a % 320);
    c.d_tabs = &tabs;
    c.kernel = int((a >> 16) % 9);
    c.dynamic = int((a >> 24) % 3) - 1;
    c.piece_auto = ((a >> 32) & 1) != 0;
    c.piece_bytes = c.piece_auto ? 128 * KiB : KiB * (1 + (a >> 40) % 1024);
    const uint64_t max_len = (b % (2 * MiB)) >> (b >> 58) % 20;   // log-spread towards 0
    const uint64_t count = (d & 0xffffffffull) >> (d >> 58) % 30;
    uint64_t total;
    switch (e % 4) {
      case 0: total = 0; break;
      case 1: total = count * max_len; break;
      case 2: total = count * ((e >> 8) % (max_len + 1)); break;  // a mean up to the hint
      default: total = (e >> 8) % (4096 * MiB); break;
    }
    check(&c, count, total, max_len);
  }
}
}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string arg = argv[i];
    if (arg == "--candidate=claim-bound") g_candidate = kClaimBound;
    else if (arg == "--candidate=ragged-order") g_candidate = kRaggedOrder;
    else if (arg == "--candidate=coop-hint") g_candidate = kCoopHint;
    else {
      std::printf("usage: route_test [--candidate=claim-bound|ragged-order|coop-hint]\n");
      return 2;
    }
  }
  grid();
  const uint64_t on_grid = g_checked;
  random_points(1000000, 0x726f757465ull);
  std::printf("%" PRIu64 " grid points, %" PRIu64 " random points; %" PRIu64 " planned; schedule static %" PRIu64
              ", guided %" PRIu64 "\n", on_grid, g_checked - on_grid, g_planned, g_sched[0], g_sched[1]);
  bool reached = g_sched[0] != 0 && g_sched[1] != 0 && g_planned != 0;
  for (Form f : {Form::Wide, Form::Narrow16, Form::Narrow8, Form::Claim, Form::Claim16, Form::Coop, Form::Sorted}) {
    std::printf("form %2d %-28s %" PRIu64 " points\n", int(f), kvsep::route::kernel_name(f), g_forms[int(f)]);
    reached = reached && g_forms[int(f)] != 0;
  }
  if (g_forms.size() != 7) reached = false;  // a form number the header does not name
  if (!reached) std::printf("UNREACHED: a form or a schedule that no point of the grid takes\n");
  std::printf("%" PRIu64 " points, %" PRIu64 " differ\n", g_checked, g_failed);
  if (g_failed || !reached) {
    std::printf("FAIL\n");
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
