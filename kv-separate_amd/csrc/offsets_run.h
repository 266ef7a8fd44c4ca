// offsets_run.h -- the geometry of the offsets pass (no HIP, no allocation: tests/cpp/offsets_run_test.cc builds it alone
// and runs the three kernels' control flow lane by lane against a plain serial loop).  The kernels (crc32c_offsets.inc)
// take every index and arithmetic decision below from here: which block a lane owns (block_index), which segments its
// run holds (concat::clamp_run, shared with the combine and the pack), how a long run is dealt to a wavefront's lanes
// (long_iters, long_seg), which blocks are kept (is_kept), a block's size and extent (block_size, extent), the wave
// scan's steps (scan_takes, row_base), the split of the tile totals into per-thread runs (scan_run, scan_range) and
// where a block lands (place, layout_end).
//
// The pass is an ordered exclusive scan of u64 extents under a keep mask:
//   dst_off[i] = start + the extents of the kept blocks before i,  extent = head + size + tail,
// with a dropped block marked kSkip.  Every addition saturates at 2^64 - 1.  Saturated sums are monotone and
// min(a + b, M) is associative, so whatever order the tiles, waves and lanes add in, the result is the serial loop's;
// a kept block whose end reaches 2^64 - 1 is marked kSkip, and so is every kept block after it (their offsets are at
// least that end).  kSkip is a value pack::fits refuses (pack_run.h), so the copy that follows skips those blocks.
#pragma once
#include <cstdint>

#include "concat_run.h"

namespace kvsep {

// The list pass of the verify forms (crc32c_verdicts.inc) has no rules header of its own; its launch geometry lives here,
// next to the tile it shares with the offsets pass, so that host-only code can include it.
constexpr uint32_t kListTile = 1024;  // blocks per tile: 4 waves x 4 rows of 64
constexpr int kListRows = 4;
constexpr uint32_t kListThreads = 256;
KVSEP_HD uint64_t list_tile_count(uint64_t count) { return (count + kListTile - 1) / kListTile; }

namespace offsets {

using concat::Run;
using concat::clamp_run;

constexpr uint32_t kTile = 1024;  // blocks per workgroup, as the verdict pass: 4 waves x 4 rows of 64
constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kWaves = 4;
constexpr uint32_t kRows = 4;
constexpr uint32_t kThreads = kWaves * kWaveLanes;
constexpr uint32_t kScanThreads = 256;  // the tile-total scan: one workgroup
static_assert(kWaves * kRows * kWaveLanes == kTile, "a tile is its waves' rows");

constexpr uint64_t kSaturated = ~uint64_t(0);
constexpr uint64_t kSkip = ~uint64_t(0);  // dst_off of a block that is not laid out
constexpr uint64_t kKeepAll = ~uint64_t(0);  // *keep_before that keeps every block

KVSEP_HD uint64_t add_sat(uint64_t a, uint64_t b) { return a + b < a ? kSaturated : a + b; }

KVSEP_HD uint64_t tile_count(uint64_t count) { return (count + kTile - 1) / kTile; }

// The pass's tile words, one array: per tile a sum, a kept count and a base, then the two grand totals.  A call over
// ntiles tiles slices it at tile_words(ntiles); an array that holds `count` blocks has scratch_words(count) words.
constexpr uint64_t kGrandWords = 2;
struct TileWords {
  uint64_t sum, kept, base, grand;
};
KVSEP_HD TileWords tile_words(uint64_t ntiles) { return {0, ntiles, 2 * ntiles, 3 * ntiles}; }
KVSEP_HD uint64_t scratch_words(uint64_t count) { return tile_words(tile_count(count)).grand + kGrandWords; }

// The block of lane `lane` in row `row` of wave `wave` of tile `tile`: consecutive lanes own consecutive blocks.
KVSEP_HD uint64_t block_index(uint64_t tile, uint32_t wave, uint32_t row, uint32_t lane) {
  return tile * kTile + (uint64_t(wave) * kRows + row) * kWaveLanes + lane;
}

// A run longer than concat::kShortMax is summed by the whole wavefront: in iteration k lane l reads segment
// s + 64 k + l (long_seg: ~0 past the run's end), long_iters iterations.
KVSEP_HD bool is_short(const Run& r) { return concat::is_short(r); }
KVSEP_HD uint64_t long_iters(const Run& r) { return (r.e - r.s + kWaveLanes - 1) / kWaveLanes; }
KVSEP_HD uint64_t long_seg(const Run& r, uint64_t k, uint32_t lane) {
  const uint64_t j = k * kWaveLanes + lane;  // < 2^64: k < long_iters
  return j < r.e - r.s ? r.s + j : ~uint64_t(0);
}

// The keep rule: mask = keep[i] (1 without a keep array), before = *keep_before (kKeepAll without one).
KVSEP_HD bool is_kept(uint8_t mask, uint64_t before, uint64_t i) { return mask != 0 && i < before; }

// A block's size from the saturated sum of its run's lengths: a sum over max_size is one no frame can hold (the vlog
// header's LE32 length), and counts as saturated -- the block and every kept block after it get kSkip.
KVSEP_HD uint64_t block_size(uint64_t sum, uint64_t max_size) { return sum > max_size ? kSaturated : sum; }

// What a block adds to the layout: head + size + tail when kept, nothing when dropped.
KVSEP_HD uint64_t extent(bool kept, uint64_t head, uint64_t size, uint64_t tail) {
  return kept ? add_sat(add_sat(head, size), tail) : 0;
}

// The inclusive wave scan: four steps within each 16-lane row, lane l adding lane l - n's value for n = 1, 2, 4, 8 when
// it has such a lane in its row (scan_takes; DPP row_shr gives the others 0), then the totals of the rows before
// (row_base) from lanes 15, 31 and 47.
constexpr uint32_t kScanSteps = 4;
constexpr uint32_t scan_shift(uint32_t step) { return 1u << step; }
KVSEP_HD bool scan_takes(uint32_t lane, uint32_t n) { return (lane & 15u) >= n; }
KVSEP_HD uint64_t row_base(uint32_t lane, uint64_t t15, uint64_t t31, uint64_t t47) {
  const uint32_t row = lane >> 4;
  const uint64_t two = add_sat(t15, t31);
  return row == 0 ? 0 : row == 1 ? t15 : row == 2 ? two : add_sat(two, t47);
}

// The tile-total scan: thread t of kScanThreads takes the contiguous tiles scan_range(t, scan_run(ntiles), ntiles).
KVSEP_HD uint64_t scan_run(uint64_t ntiles) { return (ntiles + kScanThreads - 1) / kScanThreads; }
KVSEP_HD Run scan_range(uint32_t t, uint64_t run, uint64_t ntiles) {
  const uint64_t b = uint64_t(t) * run;
  return {b < ntiles ? b : ntiles, b + run < ntiles ? b + run : ntiles};
}

// Where a block lands, from `end_incl` = start + the extents of the kept blocks up to and including it (saturated):
// a dropped block, and a kept one whose end saturated, get kSkip; else the end less the block's own extent.
KVSEP_HD uint64_t place(bool kept, uint64_t end_incl, uint64_t ext) {
  return kept && end_incl != kSaturated ? end_incl - ext : kSkip;
}

// *end of the whole layout.
KVSEP_HD uint64_t layout_end(uint64_t start, uint64_t total) { return add_sat(start, total); }

}  // namespace offsets
}  // namespace kvsep
