// chain_run_test.cc -- the rules of the chains pass (csrc/chain_run.h) on the CPU, no GPU and no library.
//
// emulate() below is the control flow of the three kernels of csrc/crc32c_logchain.inc written lane by lane over a
// memory model: every workgroup, wave, row and lane of chain_tile_kernel (two ballots a row, both incoming states,
// rows chained, the waves' summaries joined), the 256 threads of chain_scan_kernel with their two LDS scans, and
// chain_write_kernel's ballots, row and wave chaining, successor test, fragment and padding writes.  Every decision is
// a call into chain_run.h, the header the kernels and kvsep_log_chains include.  Per emulated call:
//   * first / whole / frag_off / frag_len / *nchain / *nwhole equal the documented assembly loop of
//     include/kvsep_crc32c.h restated serially (reference() below), padding included;
//   * every output element is written exactly once: first for cap + 1 elements, the others for cap, and nothing around
//     them; the words once;
//   * type / accept / gap / off / len are read at indices below min(*nrec, cap) only;
//   * every scratch word read was written earlier in the same call (a replay reads nothing stale).
// (A row that lies past both the records and the outputs votes kKeep and owns nothing; the emulation skips it.)
// Cases: every sequence of length <= 5 over {FULL, FIRST, MIDDLE, LAST, type 0, type 5, rejected} x gap {0, 1}; the same
// sequences laid across the 64-record boundaries of 3,100-record calls filled with MIDDLE (every 64-boundary of a call
// carries one, so a quarter of them cross a 256- and a sixteenth a 1,024-record boundary), and every sequence of length
// <= 3 at every straddling position of a 64-, a 256- and a 1,024-record boundary; random sequences of up to 3,100
// records at cap below, at and above the count; whole tiles of kKeep; 257 tiles.  Three deliberately wrong rules must
// each be caught.  Built with -fsanitize=address,undefined by tests/test_chain_run_cpu.py and run as it is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "chain_run.h"

using namespace kvsep;

namespace {

constexpr uint64_t kCanary = 0xC0FFEE1234567ull;
constexpr uint64_t kPad = 3;  // canary elements on each side of every output

long g_failed = 0, g_cases = 0;
std::string g_case;

struct Call {
  std::vector<uint8_t> type, accept, gap;  // min(nrec, cap) elements each: a read past them is a finding
  std::vector<uint64_t> off, len;
  bool has_gap = true, has_frag = true, want_nwhole = true;
  uint64_t nrec = 0, cap = 0;
  uint64_t count() const { return nrec < cap ? nrec : cap; }
};

struct Rules {
  bool gap_ignored_on_last = false;  // wrong: a LAST joins across a gap
  bool keep_tile_resets = false;     // wrong: a tile of only kKeep ops hands on idle
  bool first_continues = false;      // wrong: a FIRST joins the record in progress
};

struct Word {
  uint64_t v = 0;
  bool set = false;
};

template <typename T>
struct Out {
  std::vector<T> v;
  std::vector<uint8_t> writes;
  uint64_t n;
  explicit Out(uint64_t n_) : v(n_ + 2 * kPad, T(kCanary)), writes(n_ + 2 * kPad, 0), n(n_) {}
};

struct Model {
  const Call& c;
  long problems = 0;
  bool quiet;
  Out<uint64_t> first, frag_off, frag_len;
  Out<uint8_t> whole;
  uint64_t nchain = kCanary, nwhole = kCanary;
  int nchain_writes = 0, nwhole_writes = 0;
  std::vector<Word> sum, in, grand;

  Model(const Call& call, bool q)
      : c(call), quiet(q), first(call.cap + 1), frag_off(call.cap), frag_len(call.cap), whole(call.cap) {
    const uint64_t nt = chain::tile_count(c.cap);
    sum.resize(nt), in.resize(nt), grand.resize(2);
  }
  void bad(const char* what, uint64_t x = 0, uint64_t y = 0) {
    if (!quiet && g_failed + problems < 20)
      printf("FAILED %s: %s (%llu, %llu)\n", g_case.c_str(), what, (unsigned long long)x, (unsigned long long)y);
    ++problems;
  }
  template <typename T>
  T in_at(const std::vector<T>& a, uint64_t i, const char* what) {
    if (i >= c.count() || i >= a.size()) { bad(what, i); return 0; }
    return a[i];
  }
  uint8_t type_at(uint64_t i) { return in_at(c.type, i, "type[] read at or past min(*nrec, cap)"); }
  uint8_t accept_at(uint64_t i) { return in_at(c.accept, i, "accept[] read at or past min(*nrec, cap)"); }
  uint8_t gap_at(uint64_t i) { return c.has_gap ? in_at(c.gap, i, "gap[] read at or past min(*nrec, cap)") : uint8_t(0); }
  uint64_t rd(std::vector<Word>& a, uint64_t i, const char* what) {
    if (i >= a.size()) { bad(what, i); return 0; }
    if (!a[i].set) bad("a scratch word read before this call wrote it", i);
    return a[i].v;
  }
  void wr(std::vector<Word>& a, uint64_t i, uint64_t v, const char* what) {
    if (i >= a.size()) { bad(what, i); return; }
    a[i] = {v, true};
  }
  template <typename T>
  void put(Out<T>& o, uint64_t i, T v, const char* what) {
    if (i >= o.n) { bad(what, i); return; }
    o.v[kPad + i] = v;
    ++o.writes[kPad + i];
  }
};

struct Rec {
  uint8_t type = 0, accept = 0, gap = 0;
};
Rec load(Model& m, uint64_t i) { return {m.type_at(i), m.accept_at(i), m.gap_at(i)}; }

// chain::continues as the kernels call it, or one of the wrong rules in its place
bool joins_of(const Rules& rules, const Rec& r, bool in) {
  if (rules.gap_ignored_on_last && r.type == chain::kLast) return chain::continues(r.type, r.accept, 0, in);
  if (rules.first_continues && r.type == chain::kFirst && r.accept && !r.gap && in) return true;
  return chain::continues(r.type, r.accept, r.gap, in);
}

uint64_t ballot(const bool (&b)[64]) {
  uint64_t m = 0;
  for (uint32_t l = 0; l < 64; ++l) m |= uint64_t(b[l]) << l;
  return m;
}

// Rows that lie past the records and past every output own nothing and vote kKeep.
bool row_idle(const Call& c, uint64_t row_first) { return row_first >= c.count() && row_first > c.cap; }

void emulate_tile(Model& m, const Rules& rules) {
  const Call& c = m.c;
  const uint64_t nt = chain::tile_count(c.cap), count = chain::held(c.nrec, c.cap);
  for (uint64_t tile = 0; tile < nt; ++tile) {
    uint64_t wsum[chain::kWaves];
    for (uint32_t w = 0; w < chain::kWaves; ++w) {
      chain::Summary s = chain::empty_summary();
      for (uint32_t row = 0; row < chain::kRows; ++row) {
        if (row_idle(c, chain::block_index(tile, w, row, 0))) continue;
        Rec r[64];
        bool own[64], nk[64], st[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t i = chain::block_index(tile, w, row, lane);
          own[lane] = i < count;
          r[lane] = own[lane] ? load(m, i) : Rec{};
          const chain::Op op = own[lane] ? chain::op_of(r[lane].type, r[lane].accept, r[lane].gap) : chain::kKeep;
          nk[lane] = op != chain::kKeep, st[lane] = op == chain::kSet;
        }
        const uint64_t nonkeep = ballot(nk), set = ballot(st);
        chain::Summary rs;
        rs.op = chain::row_op(nonkeep, set);
        for (uint32_t h = 0; h < 2; ++h) {
          bool starts[64], wholes[64];
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const bool joins = own[lane] && joins_of(rules, r[lane], chain::state_before(h != 0, nonkeep, set, lane));
            starts[lane] = own[lane] && !joins;
            wholes[lane] = own[lane] && chain::whole_end(r[lane].type, r[lane].accept, joins);
          }
          rs.starts[h] = uint32_t(__builtin_popcountll(ballot(starts)));
          rs.wholes[h] = uint32_t(__builtin_popcountll(ballot(wholes)));
        }
        s = chain::then(s, rs);
      }
      wsum[w] = chain::pack_summary(s);
    }
    chain::Summary t = chain::empty_summary();
    for (uint32_t v = 0; v < chain::kWaves; ++v) t = chain::then(t, chain::unpack_summary(wsum[v]));
    m.wr(m.sum, tile, chain::pack_summary(t), "sum[] written past the tiles");
  }
}

chain::Op tile_op(const Rules& rules, const chain::Summary& s) {
  return rules.keep_tile_resets && s.op == chain::kKeep ? chain::kClear : s.op;
}

void emulate_scan(Model& m, const Rules& rules) {
  const uint64_t nt = chain::tile_count(m.c.cap);
  constexpr uint32_t T = chain::kScanThreads;
  static uint32_t sho[T], left[T];
  static uint64_t shc[T], shw[T], v[T], vw[T];
  static uint8_t run_in[T];
  const uint64_t run = offsets::scan_run(nt);
  std::vector<uint8_t> covered(nt, 0);
  for (uint32_t t = 0; t < T; ++t) {
    const offsets::Run r = offsets::scan_range(t, run, nt);
    chain::Op op = chain::kKeep;
    for (uint64_t i = r.s; i < r.e; ++i) {
      op = chain::compose(op, tile_op(rules, chain::unpack_summary(m.rd(m.sum, i, "sum[] read past the tiles"))));
      if (i < nt) ++covered[i];
    }
    sho[t] = op;
  }
  for (uint64_t i = 0; i < nt; ++i)
    if (covered[i] != 1) m.bad("a tile is in no thread's run, or in two", i, covered[i]);
  for (uint32_t d = 1; d < T; d <<= 1) {
    for (uint32_t t = 0; t < T; ++t) left[t] = t >= d ? sho[t - d] : uint32_t(chain::kKeep);
    for (uint32_t t = 0; t < T; ++t) sho[t] = chain::compose(chain::Op(left[t]), chain::Op(sho[t]));
  }
  for (uint32_t t = 0; t < T; ++t) {
    run_in[t] = t ? chain::apply(false, chain::Op(sho[t - 1])) : false;
    const offsets::Run r = offsets::scan_range(t, run, nt);
    uint64_t cnt = 0, wh = 0;
    bool st = run_in[t];
    for (uint64_t i = r.s; i < r.e; ++i) {
      const chain::Summary s = chain::unpack_summary(m.rd(m.sum, i, "sum[] read past the tiles"));
      cnt += s.starts[st ? 1 : 0], wh += s.wholes[st ? 1 : 0];
      st = chain::apply(st, tile_op(rules, s));
    }
    shc[t] = cnt, shw[t] = wh;
  }
  for (uint32_t d = 1; d < T; d <<= 1) {
    for (uint32_t t = 0; t < T; ++t) v[t] = t >= d ? shc[t - d] : 0, vw[t] = t >= d ? shw[t - d] : 0;
    for (uint32_t t = 0; t < T; ++t) shc[t] += v[t], shw[t] += vw[t];
  }
  for (uint32_t t = 0; t < T; ++t) {
    const offsets::Run r = offsets::scan_range(t, run, nt);
    uint64_t at = t ? shc[t - 1] : 0;
    bool st = run_in[t];
    for (uint64_t i = r.s; i < r.e; ++i) {
      const chain::Summary s = chain::unpack_summary(m.rd(m.sum, i, "sum[] read past the tiles"));
      m.wr(m.in, i, chain::pack_in(st, at), "in[] written past the tiles");
      at += s.starts[st ? 1 : 0];
      st = chain::apply(st, tile_op(rules, s));
    }
  }
  m.wr(m.grand, 0, shc[T - 1], "grand");
  m.wr(m.grand, 1, shw[T - 1], "grand");
}

void emulate_write(Model& m, const Rules& rules) {
  const Call& c = m.c;
  const uint64_t nt = chain::tile_count(c.cap), count = chain::held(c.nrec, c.cap);
  for (uint64_t tile = 0; tile < chain::write_tiles(c.cap); ++tile) {
    const bool has = tile < nt;
    uint64_t nchain = 0, nwhole = 0;
    if (nt) nchain = m.rd(m.grand, 0, "grand"), nwhole = m.rd(m.grand, 1, "grand");
    static Rec rec[chain::kWaves][chain::kRows][64], nx[chain::kWaves][chain::kRows][64];
    static uint64_t off[chain::kWaves][chain::kRows][64], len[chain::kWaves][chain::kRows][64];
    static bool own[chain::kWaves][chain::kRows][64], joins[chain::kWaves][chain::kRows][64],
        after[chain::kWaves][chain::kRows][64];
    static uint32_t rank[chain::kWaves][chain::kRows][64];
    uint64_t nonkeep[chain::kWaves][chain::kRows] = {}, set[chain::kWaves][chain::kRows] = {};
    uint32_t wop[chain::kWaves] = {}, wst[chain::kWaves] = {};
    uint64_t tin = 0;
    if (has) {
      tin = m.rd(m.in, tile, "in[] read past the tiles");
      for (uint32_t w = 0; w < chain::kWaves; ++w) {  // up to the first workgroup barrier
        chain::Op mine = chain::kKeep;
        for (uint32_t row = 0; row < chain::kRows; ++row) {
          if (row_idle(c, chain::block_index(tile, w, row, 0))) {
            for (uint32_t lane = 0; lane < 64; ++lane) own[w][row][lane] = false;
            continue;
          }
          bool nk[64], st[64];
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t i = chain::block_index(tile, w, row, lane);
            const bool o = own[w][row][lane] = i < count;
            rec[w][row][lane] = nx[w][row][lane] = Rec{};
            off[w][row][lane] = len[w][row][lane] = 0;
            if (o) {
              rec[w][row][lane] = load(m, i);
              nx[w][row][lane] = load(m, chain::next_index(i, count));
              if (c.has_frag) {
                off[w][row][lane] = m.in_at(c.off, i, "off[] read at or past min(*nrec, cap)");
                len[w][row][lane] = m.in_at(c.len, i, "len[] read at or past min(*nrec, cap)");
              }
            }
            const Rec& r = rec[w][row][lane];
            const chain::Op op = o ? chain::op_of(r.type, r.accept, r.gap) : chain::kKeep;
            nk[lane] = op != chain::kKeep, st[lane] = op == chain::kSet;
          }
          nonkeep[w][row] = ballot(nk), set[w][row] = ballot(st);
          mine = chain::compose(mine, chain::row_op(nonkeep[w][row], set[w][row]));
        }
        wop[w] = mine;
      }
      for (uint32_t w = 0; w < chain::kWaves; ++w) {  // up to the second
        bool in = chain::in_state(tin);
        for (uint32_t u = 0; u < w; ++u) in = chain::apply(in, chain::Op(wop[u]));
        uint32_t starts = 0;
        for (uint32_t row = 0; row < chain::kRows; ++row) {
          if (row_idle(c, chain::block_index(tile, w, row, 0))) continue;
          bool sbv[64];
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const Rec& r = rec[w][row][lane];
            const bool o = own[w][row][lane];
            const bool st = chain::state_before(in, nonkeep[w][row], set[w][row], lane);
            joins[w][row][lane] = o && joins_of(rules, r, st);
            after[w][row][lane] = chain::apply(st, o ? chain::op_of(r.type, r.accept, r.gap) : chain::kKeep);
            sbv[lane] = o && !joins[w][row][lane];
          }
          const uint64_t sb = ballot(sbv);
          for (uint32_t lane = 0; lane < 64; ++lane)
            rank[w][row][lane] =
                starts + uint32_t(__builtin_popcountll(sb & chain::lanes_below(lane))) + (sbv[lane] ? 1u : 0u);
          starts += uint32_t(__builtin_popcountll(sb));
          in = chain::state_after_row(in, nonkeep[w][row], set[w][row]);
        }
        wst[w] = starts;
      }
    }
    for (uint32_t w = 0; w < chain::kWaves; ++w) {
      uint64_t before = 0;
      if (has) {
        before = chain::in_base(tin);
        for (uint32_t u = 0; u < w; ++u) before += wst[u];
      }
      for (uint32_t row = 0; row < chain::kRows; ++row) {
        if (row_idle(c, chain::block_index(tile, w, row, 0))) continue;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t k = chain::block_index(tile, w, row, lane);
          if (has && own[w][row][lane]) {
            const uint64_t j = chain::chain_of(before, rank[w][row][lane]);
            const Rec& r = rec[w][row][lane];
            const Rec& n = nx[w][row][lane];
            if (!joins[w][row][lane] && j <= c.cap) m.put(m.first, j, k, "first[] written past cap + 1 elements");
            if (chain::chain_ends(k, count, joins_of(rules, n, after[w][row][lane])) && j < c.cap)
              m.put(m.whole, j, uint8_t(chain::whole_end(r.type, r.accept, joins[w][row][lane]) ? 1 : 0),
                    "whole[] written past cap elements");
            if (c.has_frag) {
              m.put(m.frag_off, k, chain::frag_off(off[w][row][lane]), "frag_off[] written past cap elements");
              m.put(m.frag_len, k, chain::frag_len(len[w][row][lane]), "frag_len[] written past cap elements");
            }
          }
          if (chain::pads_first(k, nchain, c.cap)) m.put(m.first, k, chain::pad_first(count), "first[] padding past cap + 1");
          if (chain::pads_whole(k, nchain, c.cap)) m.put(m.whole, k, uint8_t(0), "whole[] padding past cap");
          if (c.has_frag && chain::pads_frag(k, count, c.cap)) {
            m.put(m.frag_off, k, uint64_t(0), "frag_off[] padding past cap");
            m.put(m.frag_len, k, uint64_t(0), "frag_len[] padding past cap");
          }
        }
      }
    }
    if (tile == 0) {
      m.nchain = nchain, ++m.nchain_writes;
      if (c.want_nwhole) m.nwhole = nwhole, ++m.nwhole_writes;
    }
  }
}

// The documented loop (include/kvsep_crc32c.h, at kvsep_log_accept_gaps), read independently: one serial pass with
// `in_fragment`.  A record that is not appended to the record in progress opens a new chain; a chain is whole when the
// loop returns a record at its last element.
struct Want {
  std::vector<uint64_t> first;
  std::vector<uint8_t> whole;
  uint64_t nchain = 0, nwhole = 0;
};
Want reference(const Call& c) {
  const uint64_t count = c.count();
  Want w;
  w.first.assign(c.cap + 1, count);
  w.whole.assign(c.cap, 0);
  bool in_fragment = false;
  for (uint64_t i = 0; i < count; ++i) {
    const uint8_t t = c.type[i], a = c.accept[i], g = c.has_gap ? c.gap[i] : 0;
    if (g || !a) in_fragment = false;  // drop the record in progress
    bool appended = false, returned = false;
    if (a) {
      switch (t) {
        case 1: in_fragment = false, returned = true; break;           // FULL: return payload i
        case 2: in_fragment = true; break;                            // FIRST: start a record
        case 3: appended = in_fragment; break;                         // MIDDLE: append when one is in progress
        case 4: appended = returned = in_fragment, in_fragment = false; break;  // LAST: append and return it
        default: in_fragment = false; break;                           // unknown record type
      }
    }
    if (!appended) w.first[w.nchain++] = i;
    if (returned) w.whole[w.nchain - 1] = 1, ++w.nwhole;
  }
  return w;
}

template <typename T>
void check_out(Model& m, const Out<T>& o, bool written, const char* name) {
  for (uint64_t i = 0; i < o.n; ++i)
    if (o.writes[kPad + i] != (written ? 1 : 0)) m.bad(name, i, o.writes[kPad + i]);
  for (uint64_t k = 0; k < kPad; ++k)
    if (o.v[k] != T(kCanary) || o.v[kPad + o.n + k] != T(kCanary) || o.writes[k] || o.writes[kPad + o.n + k])
      m.bad("an element around an output was written", k);
}

long run_case(const Call& c, const Rules& rules, bool quiet) {
  Model m(c, quiet);
  if (c.cap) {
    emulate_tile(m, rules);
    emulate_scan(m, rules);
  }
  emulate_write(m, rules);
  const Want w = reference(c);
  check_out(m, m.first, true, "first[] element not written exactly once");
  check_out(m, m.whole, true, "whole[] element not written exactly once");
  check_out(m, m.frag_off, c.has_frag, "frag_off[] element not written as the call asks");
  check_out(m, m.frag_len, c.has_frag, "frag_len[] element not written as the call asks");
  for (uint64_t j = 0; j <= c.cap; ++j)
    if (m.first.v[kPad + j] != w.first[j]) m.bad("first[j] differs from the serial loop", j, m.first.v[kPad + j]);
  for (uint64_t j = 0; j < c.cap; ++j)
    if (m.whole.v[kPad + j] != w.whole[j]) m.bad("whole[j] differs from the serial loop", j, m.whole.v[kPad + j]);
  if (c.has_frag)
    for (uint64_t i = 0; i < c.cap; ++i) {
      const uint64_t fo = i < c.count() ? c.off[i] + 1 : 0, fl = i < c.count() ? c.len[i] - 1 : 0;
      if (m.frag_off.v[kPad + i] != fo || m.frag_len.v[kPad + i] != fl) m.bad("frag_off / frag_len", i);
    }
  if (m.nchain_writes != 1 || m.nchain != w.nchain) m.bad("*nchain", m.nchain, w.nchain);
  if (c.want_nwhole ? (m.nwhole_writes != 1 || m.nwhole != w.nwhole) : (m.nwhole_writes != 0 || m.nwhole != kCanary))
    m.bad("*nwhole", m.nwhole, w.nwhole);
  return m.problems;
}

// The alphabet: 7 record kinds x gap.
constexpr uint32_t kSymbols = 14;
void symbol(uint32_t s, uint8_t& type, uint8_t& accept, uint8_t& gap) {
  static const uint8_t types[7] = {1, 2, 3, 4, 0, 5, 3};
  type = types[s % 7], accept = s % 7 == 6 ? 0 : 1, gap = uint8_t(s / 7);
}

// Gives the arrays their walk entries and cuts them to min(nrec, cap).
Call finish(std::vector<uint8_t> type, std::vector<uint8_t> accept, std::vector<uint8_t> gap, uint64_t cap, uint64_t salt) {
  Call c;
  c.nrec = type.size(), c.cap = cap;
  const uint64_t count = c.count();
  type.resize(count), accept.resize(count), gap.resize(count);
  c.type = type, c.accept = accept, c.gap = gap;
  c.off.resize(count), c.len.resize(count);
  for (uint64_t i = 0; i < count; ++i) c.off[i] = 6 + i * 40 + salt % 7, c.len[i] = 1 + (i * 2654435761u + salt) % 33;
  c.has_frag = salt % 5 != 0, c.want_nwhole = salt % 3 != 0;
  return c;
}

uint64_t cap_for(uint64_t n, uint64_t pick) { return pick % 3 == 0 ? n : pick % 3 == 1 ? (n ? n - 1 : 0) : n + 3; }

// The cases, each given to `visit`.  `full`: the exhaustive sets of length 4 and 5 too (the right rules only).
template <typename Visit>
void all_cases(bool full, Visit visit) {
  std::mt19937_64 rng(20261020);
  const uint32_t max_len = full ? 5 : 3;
  std::vector<std::vector<uint32_t>> seqs;  // every sequence of length <= max_len, by length
  for (uint32_t n = 0; n <= max_len; ++n) {
    uint64_t total = 1;
    for (uint32_t k = 0; k < n; ++k) total *= kSymbols;
    for (uint64_t x = 0; x < total; ++x) {
      std::vector<uint32_t> s(n);
      uint64_t y = x;
      for (uint32_t k = 0; k < n; ++k) s[k] = uint32_t(y % kSymbols), y /= kSymbols;
      seqs.push_back(s);
    }
  }
  // alone
  for (uint64_t q = 0; q < seqs.size(); ++q) {
    const auto& s = seqs[q];
    std::vector<uint8_t> t(s.size()), a(s.size()), g(s.size());
    for (uint64_t k = 0; k < s.size(); ++k) symbol(s[k], t[k], a[k], g[k]);
    visit(finish(t, a, g, cap_for(s.size(), q), q), "sequence #" + std::to_string(q));
  }
  // a 3,100-record call of MIDDLE, in progress (a FIRST at 0) or not, with `put` laying sequences into it
  auto filler = [&](bool in_progress, std::vector<uint8_t>& t, std::vector<uint8_t>& a, std::vector<uint8_t>& g) {
    t.assign(3100, 3), a.assign(3100, 1), g.assign(3100, 0);
    if (in_progress) t[0] = 2;
  };
  auto put = [&](const std::vector<uint32_t>& s, uint64_t at, std::vector<uint8_t>& t, std::vector<uint8_t>& a,
                 std::vector<uint8_t>& g) {
    for (uint64_t k = 0; k < s.size(); ++k) symbol(s[k], t[at + k], a[at + k], g[at + k]);
  };
  // across the 64-record boundaries: boundary b of call q / 48 carries sequence q, one to |s| records before it
  for (uint64_t q = 0; q < seqs.size(); q += 48) {
    std::vector<uint8_t> t, a, g;
    filler((q / 48) % 2 == 0, t, a, g);
    for (uint64_t b = 1; b <= 48 && q + b - 1 < seqs.size(); ++b) {
      const auto& s = seqs[q + b - 1];
      if (s.empty()) continue;
      put(s, b * 64 - (1 + (q + b) % s.size()), t, a, g);
    }
    visit(finish(t, a, g, cap_for(3100, q / 48), q), "sequences from #" + std::to_string(q) + " across the 64-boundaries");
  }
  // every sequence of length <= 3 at every straddling position of a 64-, a 256- and a 1,024-record boundary
  for (uint64_t q = 0; q < seqs.size() && seqs[q].size() <= 3; ++q)
    for (uint64_t boundary : {64ull, 256ull, 1024ull})
      for (uint64_t back = 0; back <= seqs[q].size(); ++back) {
        if (seqs[q].empty()) continue;
        std::vector<uint8_t> t, a, g;
        filler((q + back) % 2 == 0, t, a, g);
        t.resize(boundary + 70), a.resize(boundary + 70), g.resize(boundary + 70);
        put(seqs[q], boundary - back, t, a, g);
        t.back() = 4;  // the LAST that ends the run
        visit(finish(t, a, g, cap_for(t.size(), q + back), q),
              "sequence #" + std::to_string(q) + " at " + std::to_string(boundary) + " - " + std::to_string(back));
      }
  // whole tiles of kKeep: one FIRST, MIDDLE to the end, with and without the LAST; and idle throughout
  for (uint64_t n : {1024ull, 1025ull, 2049ull, 3100ull})
    for (int mode = 0; mode < 3; ++mode)
      for (uint64_t pick = 0; pick < 3; ++pick) {
        std::vector<uint8_t> t(n, 3), a(n, 1), g(n, 0);
        if (mode != 2) t[0] = 2;
        if (mode == 0) t[n - 1] = 4;
        Call c = finish(t, a, g, cap_for(n, pick), n + mode);
        c.has_gap = mode != 1;
        visit(c, "a run of MIDDLE, " + std::to_string(n) + " records, mode " + std::to_string(mode));
      }
  // random sequences of up to 3,100 records, weighted towards MIDDLE, at cap below, at and above the count
  for (int x = 0; x < 120; ++x) {
    const uint64_t n = x < 6 ? uint64_t(x) : x % 10 == 0 ? 3100 : rng() % 3101;
    std::vector<uint8_t> t(n), a(n), g(n);
    const uint32_t heavy = x % 4;  // 0: uniform; else MIDDLE three times in four
    for (uint64_t i = 0; i < n; ++i) {
      uint32_t s = uint32_t(rng() % kSymbols);
      if (heavy && rng() % 4) s = 2;
      symbol(s, t[i], a[i], g[i]);
      if (x % 7 == 3) g[i] = 0;
    }
    for (uint64_t pick = 0; pick < 3; ++pick) {
      Call c = finish(t, a, g, cap_for(n, pick), uint64_t(x));
      c.has_gap = x % 7 != 3;
      visit(c, "random #" + std::to_string(x) + " cap " + std::to_string(c.cap));
    }
  }
  {  // *nrec far over cap, cap == 0 with records, and no records at all
    std::vector<uint8_t> t(500, 3), a(500, 1), g(500, 0);
    t[0] = 2, t[70] = 4, t[71] = 1;
    visit(finish(t, a, g, 72, 1), "*nrec 500, cap 72");
    visit(finish(t, a, g, 0, 1), "*nrec 500, cap 0");
    visit(finish({}, {}, {}, 0, 1), "nothing");
    visit(finish({}, {}, {}, 1030, 1), "no records, cap 1,030");
  }
  if (full) {  // more than 256 tiles: the scan kernel's per-thread runs hold two tiles
    const uint64_t n = 262145 + 700;
    std::vector<uint8_t> t(n), a(n), g(n);
    for (uint64_t i = 0; i < n; ++i) {
      uint32_t s = uint32_t(rng() % kSymbols);
      if (rng() % 64) s = 2;
      symbol(s, t[i], a[i], g[i]);
    }
    visit(finish(t, a, g, n, 2), "257 tiles");
  }
}

}  // namespace

int main() {
  all_cases(true, [](const Call& c, const std::string& name) {
    g_case = name;
    ++g_cases;
    g_failed += run_case(c, Rules{}, false);
  });
  // the model must catch each wrong rule somewhere in the smaller case set
  const char* names[3] = {"gap ignored on a LAST", "a tile of only KEEP ops that resets the incoming state",
                          "a FIRST that continues the chain before it"};
  for (int w = 0; w < 3; ++w) {
    Rules r;
    r.gap_ignored_on_last = w == 0, r.keep_tile_resets = w == 1, r.first_continues = w == 2;
    long caught = 0;
    all_cases(false, [&](const Call& c, const std::string&) { caught += run_case(c, r, true) ? 1 : 0; });
    printf("wrong rule (%s): caught in %ld cases\n", names[w], caught);
    if (!caught) {
      printf("FAILED: the model did not catch %s\n", names[w]);
      ++g_failed;
    }
  }
  printf("%ld emulated calls\n", g_cases);
  printf("%s: %ld cases, %ld failed\n", g_failed ? "FAIL" : "PASS", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
