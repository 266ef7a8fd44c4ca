// chain_run.h -- the rules of the chains pass (no HIP, no allocation: tests/cpp/chain_run_test.cc builds it alone and
// runs the three kernels' control flow lane by lane against the documented assembly loop restated serially).  The
// kernels (crc32c_logchain.inc) and kvsep_log_chains (framing.cpp) take every decision below from here: what a record
// does to the assembly state (op_of, compose, apply), whether it joins the chain before it (continues), whether it is
// its chain's last record and whether that chain is whole (next_index, chain_ends, whole_end), how a row of 64 records
// is resolved from two ballots (row_op, state_before, state_after_row), a tile's summary and what it gives for an
// incoming state (Summary, then, pack_summary, unpack_summary, pack_in, in_state, in_base), the per-thread runs of the
// tile scan (offsets::scan_run, scan_range, shared with the offsets pass), the fragment descriptors (frag_off,
// frag_len) and the padding (pads_first, pads_whole, pads_frag, pad_first).
//
// The assembly of log::Reader::ReadRecord (db/log_reader.cc:60-172; the loop in include/kvsep_crc32c.h) keeps one bit,
// "a record is in progress", and a scratch string.  Over record indices that is a one-bit state machine:
//
//   record i                             state after   joins the chain before it
//   accept[i] == 0                       idle          no
//   accepted FIRST, any gap              in            no
//   accepted MIDDLE, gap[i] == 0         unchanged     iff the state before is `in`
//   accepted MIDDLE, gap[i] == 1         idle          no
//   accepted LAST                        idle          iff gap[i] == 0 and the state before is `in`
//   accepted FULL / any other type       idle          no
//
// A record that does not join starts a new chain, so the chains cut [0, count) into runs of consecutive records.  A
// chain is whole -- a record the reader returns -- iff its last record is an accepted FULL (the chain is that record) or
// a LAST that joined; its records are then the record's fragments, in order.  Every other chain is dropped.  The ops
// compose as "the rightmost one that is not kKeep wins", which is associative: the state before each record is an
// exclusive scan, and inside a wavefront two ballots and the highest set bit below the lane.
#pragma once
#include <cstdint>

#include "offsets_run.h"  // KVSEP_HD, the tile geometry and the scan runs

namespace kvsep {
namespace chain {

constexpr uint8_t kFull = 1, kFirst = 2, kMiddle = 3, kLast = 4;  // db/log_format.h:16-24

using offsets::kTile;
using offsets::kWaves;
using offsets::kRows;
using offsets::kThreads;
using offsets::kScanThreads;
using offsets::tile_count;
using offsets::block_index;

// *nrec clamped to the arrays' capacity, once: every index of the pass is below it.
KVSEP_HD uint64_t held(uint64_t nrec, uint64_t cap) { return nrec < cap ? nrec : cap; }

// ---- the state machine
enum Op : uint32_t { kKeep = 0, kClear = 1, kSet = 2 };

KVSEP_HD Op op_of(uint8_t type, uint8_t accept, uint8_t gap) {
  if (!accept) return kClear;
  if (type == kFirst) return kSet;
  if (type == kMiddle && !gap) return kKeep;
  return kClear;
}
// `a`, then `b`.
KVSEP_HD Op compose(Op a, Op b) { return b != kKeep ? b : a; }
KVSEP_HD bool apply(bool in, Op o) { return o == kKeep ? in : o == kSet; }
// Does the record join the chain before it, `in` being the state before it.
KVSEP_HD bool continues(uint8_t type, uint8_t accept, uint8_t gap, bool in) {
  return accept && !gap && (type == kMiddle || type == kLast) && in;
}
// The successor whose three bytes decide whether record i ends its chain, never outside [0, count) (count != 0).
KVSEP_HD uint64_t next_index(uint64_t i, uint64_t count) { return i + 1 < count ? i + 1 : count - 1; }
// Record i is its chain's last: the arrays end with it, or the record after it starts a chain.
KVSEP_HD bool chain_ends(uint64_t i, uint64_t count, bool next_continues) { return i + 1 >= count || !next_continues; }
// Is the chain whose last record this is whole: `continued` = the record joined the chain before it.
KVSEP_HD bool whole_end(uint8_t type, uint8_t accept, bool continued) {
  return accept && (type == kFull || (type == kLast && continued));
}

// ---- a row of 64 consecutive records from two ballots: nonkeep = the lanes whose op is not kKeep, set = those whose
// op is kSet.  A lane past the records votes kKeep.
KVSEP_HD uint32_t top_bit(uint64_t m) { return 63u - uint32_t(__builtin_clzll(m)); }  // m != 0
KVSEP_HD Op row_op(uint64_t nonkeep, uint64_t set) {
  return !nonkeep ? kKeep : (set >> top_bit(nonkeep)) & 1 ? kSet : kClear;
}
KVSEP_HD uint64_t lanes_below(uint32_t lane) { return (uint64_t(1) << lane) - 1; }
// The state before lane `lane`, row_in being the state before lane 0.
KVSEP_HD bool state_before(bool row_in, uint64_t nonkeep, uint64_t set, uint32_t lane) {
  return apply(row_in, row_op(nonkeep & lanes_below(lane), set));
}
KVSEP_HD bool state_after_row(bool row_in, uint64_t nonkeep, uint64_t set) { return apply(row_in, row_op(nonkeep, set)); }

// ---- a run of records summarised: its composed op, and for an incoming state of idle ([0]) and of `in` ([1]) how many
// chains start in it and how many whole chains end in it.  The two differ only through the records before the run's
// first op that is not kKeep, and through that record itself when it is a LAST.
struct Summary {
  Op op;
  uint32_t starts[2], wholes[2];
};
KVSEP_HD Summary empty_summary() { return {kKeep, {0, 0}, {0, 0}}; }
// `a`, then `b`: b's incoming state is what a leaves.
KVSEP_HD Summary then(const Summary& a, const Summary& b) {
  Summary r;
  r.op = compose(a.op, b.op);
  for (uint32_t h = 0; h < 2; ++h) {
    const uint32_t mid = apply(h != 0, a.op) ? 1u : 0u;
    r.starts[h] = a.starts[h] + b.starts[mid];
    r.wholes[h] = a.wholes[h] + b.wholes[mid];
  }
  return r;
}
// A tile's summary in one scratch word: the counts are at most kTile.
constexpr uint32_t kCountBits = 11;
static_assert(kTile < (1u << kCountBits), "a tile's counts fit their fields");
KVSEP_HD uint64_t pack_summary(const Summary& s) {
  return uint64_t(s.op) | uint64_t(s.starts[0]) << 2 | uint64_t(s.starts[1]) << (2 + kCountBits) |
         uint64_t(s.wholes[0]) << (2 + 2 * kCountBits) | uint64_t(s.wholes[1]) << (2 + 3 * kCountBits);
}
KVSEP_HD Summary unpack_summary(uint64_t w) {
  constexpr uint64_t m = (uint64_t(1) << kCountBits) - 1;
  return {Op(w & 3), {uint32_t(w >> 2 & m), uint32_t(w >> (2 + kCountBits) & m)},
          {uint32_t(w >> (2 + 2 * kCountBits) & m), uint32_t(w >> (2 + 3 * kCountBits) & m)}};
}
// What the tile scan hands a tile: its incoming state and the number of chains that start before it (< 2^32).
KVSEP_HD uint64_t pack_in(bool in, uint64_t base) { return base << 1 | (in ? 1 : 0); }
KVSEP_HD bool in_state(uint64_t w) { return w & 1; }
KVSEP_HD uint64_t in_base(uint64_t w) { return w >> 1; }
// Chain of a record: `before` = the chains that start before its tile (and, in the write kernel, its wave), `rank` = the
// starts among the records from there up to and including it.  Record 0 always starts a chain, so this is never -1.
KVSEP_HD uint64_t chain_of(uint64_t before, uint32_t rank) { return before + rank - 1; }

// ---- fragments and padding
// The walk's off is the type byte and its len 1 + payload.  (A length of 0, which no walk gives, has no payload.)
KVSEP_HD uint64_t frag_off(uint64_t off) { return off + 1; }
KVSEP_HD uint64_t frag_len(uint64_t len) { return len ? len - 1 : 0; }
// Element k of the outputs when no record / chain owns it: first[] holds `count` from nchain to cap inclusive, whole[]
// 0 from nchain to cap, frag_off / frag_len 0 from count to cap.
KVSEP_HD bool pads_first(uint64_t k, uint64_t nchain, uint64_t cap) { return k >= nchain && k <= cap; }
KVSEP_HD bool pads_whole(uint64_t k, uint64_t nchain, uint64_t cap) { return k >= nchain && k < cap; }
KVSEP_HD bool pads_frag(uint64_t k, uint64_t count, uint64_t cap) { return k >= count && k < cap; }
KVSEP_HD uint64_t pad_first(uint64_t count) { return count; }
// The write kernel's grid: a lane per element of first[], the longest output (cap + 1).
KVSEP_HD uint64_t write_tiles(uint64_t cap) { return tile_count(cap + 1); }
// chain_reclen_kernel's grid: a lane per chain.
KVSEP_HD uint64_t reclen_grid(uint64_t cap) { return (cap + kThreads - 1) / kThreads; }

// The pass's scratch words, one array: per tile of records its summary and what the scan hands it, then the two grand
// totals.  A call over ntiles tiles slices it at tile_words(ntiles); an array that holds cap records has
// scratch_words(cap) words.
constexpr uint64_t kGrandWords = 2;
struct TileWords {
  uint64_t sum, in, grand;
};
KVSEP_HD TileWords tile_words(uint64_t ntiles) { return {0, ntiles, 2 * ntiles}; }
KVSEP_HD uint64_t scratch_words(uint64_t cap) { return tile_words(tile_count(cap)).grand + kGrandWords; }

}  // namespace chain
}  // namespace kvsep
