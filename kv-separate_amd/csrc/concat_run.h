// concat_run.h -- the run arithmetic of crc32c_concat_kernel (no HIP, no allocation: tests/cpp/concat_run_test.cc builds
// it alone and runs it against a plain serial fold, malformed first[] included).  The kernel (crc32c_concat.inc) and the
// host fold of the gather forms take every index decision below from here: which segments a block's run holds
// (clamp_run), how a long run is cut into passes of a wavefront and into one contiguous chunk per lane (pass_end,
// lane_chunk, lane_range), which lanes join at each level of the ordered lane tree (tree_joins, tree_partner), and the
// operator that joins two folded pieces (compose).
//
// A segment j of a run is the affine map c -> c * X(seg_len[j]) ^ seg_crc[j] on the CRC value (X(n) = x^(8n) mod P,
// gf2.h): Extend(c, B) = c * X(|B|) ^ Value(B), the pre- and post-inversions cancel.  A run is the composition of its
// segments' maps in order; multipliers are composed, lengths are never added (their sums overflow 64 bits).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KVSEP_HD __host__ __device__ inline
#else
#define KVSEP_HD inline
#endif

namespace kvsep {

// crc32c_concat_kernel's workgroup (crc32c_concat.inc); here so that host-only code can include it.
constexpr uint32_t kConcatThreads = 256;
constexpr uint32_t kConcatWaves = kConcatThreads / 64;

namespace concat {

// A run of up to kShortMax segments is folded serially by one lane, a longer one by a whole wavefront.  One lane's fold
// costs one carry-less product per segment; the wavefront's costs two per segment of a lane's chunk plus twelve for the
// tree, on 64 lanes.  At 32 segments the serial fold is at 2.5x the wavefront's latency for 1/26 of its lane work; from
// there on its latency grows by a product per segment while the wavefront's stays flat up to 64, so longer runs get
// the wavefront.  Per lane-work the serial fold wins at every length: the threshold buys latency, for batches whose few
// long runs would otherwise each hold one lane for a product per segment.
constexpr uint64_t kShortMax = 32;
// Blocks per wavefront: lanes [0, kWaveBlocks) each read one block's run.  Fewer than 64, so that the long runs one
// wavefront has to take one after another stay few.  Measured at 16 and at 4 (profiles/round8/gather_cost.txt): 4 halves
// the time of a batch of nothing but long runs (186 -> 95 us for 16,384 runs of 64) and doubles the time of a batch of
// one-segment blocks (5 -> 11 us for 65,536), the case the gather form meets most; 16 stays.
constexpr uint32_t kWaveBlocks = 16;
constexpr uint32_t kWaveLanes = 64;
// Blocks per workgroup, and the grid of a batch of `count` blocks.
constexpr uint64_t kPerWg = uint64_t(kConcatWaves) * kWaveBlocks;
KVSEP_HD uint64_t grid_for(uint64_t count) { return (count + kPerWg - 1) / kPerWg; }
// Segments one lane folds in one pass of a long run: a pass covers up to kPassSegs segments, so the lanes' chunks of
// one pass sit within 12 KiB of seg_len / seg_crc.
constexpr uint64_t kLaneSegs = 16;
constexpr uint64_t kPassSegs = kWaveLanes * kLaneSegs;
constexpr int kTreeLevels = 6;

constexpr uint32_t kOne = 0x80000000u;  // x^0 in the reflected representation

// Segments [s, e) of seg_crc / seg_len.
struct Run {
  uint64_t s, e;
};

// Block i's run from first[i], first[i + 1]: both clamped to nseg, and a run that ends before it starts is empty.  So
// whatever first[] holds, s <= e <= nseg: no segment index taken from it leaves the arrays.
KVSEP_HD Run clamp_run(uint64_t f0, uint64_t f1, uint64_t nseg) {
  const uint64_t s = f0 < nseg ? f0 : nseg;
  const uint64_t e = f1 < nseg ? f1 : nseg;
  return {s, e < s ? s : e};
}

KVSEP_HD bool is_short(const Run& r) { return r.e - r.s <= kShortMax; }

// A long run goes through the wavefront in passes [ps, pass_end(ps, e)) of at most kPassSegs segments.
KVSEP_HD uint64_t pass_end(uint64_t ps, uint64_t e) { return e - ps < kPassSegs ? e : ps + kPassSegs; }

// Segments per lane of a pass of n segments (1 <= n <= kPassSegs): ceil(n / 64), so 64 chunks cover the pass.
KVSEP_HD uint64_t lane_chunk(uint64_t n) { return (n + kWaveLanes - 1) / kWaveLanes; }

// Lane `lane`'s chunk of the pass [ps, pe): contiguous, in lane order, clipped to the pass; the lanes past the end of
// a short pass get an empty chunk (and carry the identity).
KVSEP_HD Run lane_range(uint64_t ps, uint64_t pe, uint64_t chunk, uint32_t lane) {
  const uint64_t n = pe - ps;
  const uint64_t a = uint64_t(lane) * chunk, b = a + chunk;
  return {ps + (a < n ? a : n), ps + (b < n ? b : n)};
}

// The affine map c -> c * m ^ v.
struct Pair {
  uint32_t m, v;
};
KVSEP_HD Pair identity() { return {kOne, 0u}; }

// `a` first, then `b`: (c * a.m ^ a.v) * b.m ^ b.v.  Associative, not commutative.  mul is the product mod P.
template <typename Mul>
KVSEP_HD Pair compose(const Pair& a, const Pair& b, Mul mul) {
  return {mul(a.m, b.m), mul(a.v, b.m) ^ b.v};
}

// The ordered tree over the 64 lanes' pairs: at level k (0 .. 5) the lanes whose low k + 1 bits are all ones replace
// their pair by compose(pair of lane - 2^k, own pair); after level 5 lane 63 holds the pass.
KVSEP_HD bool tree_joins(uint32_t lane, int level) {
  const uint32_t m = (2u << level) - 1u;
  return (lane & m) == m;
}
KVSEP_HD uint32_t tree_partner(uint32_t lane, int level) { return lane - (1u << level); }

}  // namespace concat
}  // namespace kvsep
