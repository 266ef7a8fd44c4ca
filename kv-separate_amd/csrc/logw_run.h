// logw_run.h -- the rules of the log / MANIFEST write side (no HIP, no allocation: tests/cpp/logw_run_test.cc builds it
// alone and runs the two kernels' control flow lane by lane against log::Writer::AddRecord's loop restated serially).
// The kernels (crc32c_logframe.inc) and kvsep_log_frame_layout (framing.cpp) take every decision below from here: what a
// record does to the writer's block offset (start_state, after, resets, pad_bytes, start_of), how a length is reduced so
// that a row of 64 records scans in 32 bits (reduce, step_of, join), how a row is resolved (row_u, raw_before, raw_behind,
// commit_mask, lanes_upto), how many fragments a record has and how many blocks it advances (nfrag, blocks_advanced),
// where it lands (pos_sat, rel, laid, rec_at), what each of its fragments is (frag_begin, frag_len, frag_at, frag_type),
// which record owns a fragment slot (owner), the scratch word (pack_rec, rec_b, rec_pad) and the padding (pads_frag,
// pad_*).
//
// log::Writer::AddRecord (db/log_writer.cc:35-82) keeps one number, block_offset_ in [0, 32768].  Before each fragment
// it looks at leftover = 32768 - block_offset_: under 7 bytes it zero-fills them and starts a block.  A fragment then
// takes min(left, 32768 - block_offset_ - 7) payload bytes behind a 7-byte header.  Over records, not fragments:
//
//   raw      the offset a record leaves behind, in [0, 32768]; dest_length % 32768 before the first one
//   resets   raw > 32761: the NEXT record starts a block, behind 32768 - raw zero bytes (none for raw = 32768).  The
//            zeros belong to that next record -- the pad is lazy, no trailer follows the last record of a call
//   b        the offset the record's first header goes to: 0 after a reset, else raw;  b <= 32761
//   U        b + 7 + len
//   after(U) the raw the record leaves: U when U <= 32768 (one fragment, possibly filling the block exactly); otherwise
//            the first fragment fills its block, R = U - 32768 >= 1 payload bytes follow in fragments of 32761, the last
//            of them ((R - 1) mod 32761) + 1 bytes behind its header: 8 + (U - 32769) mod 32761
//
// A record that leaves a raw <= 32761 hands b = raw to the next one, and after(after(U) + x) = after(U + x): for
// U <= 32768 trivially; else after(U) = 8 + m with m = (U - 32769) mod 32761, and 8 + m + x is either <= 32768, which
// is m + x < 32761 so that after(U + x) = 8 + (m + x) mod 32761 = 8 + m + x, or larger, where both sides are
// 8 + (m + x - 32761) mod 32761.  So until a reset the raw after a record is after(b0 + the sum of 7 + len since b0),
// a function of a running sum: a wavefront scans 64 records at once, ballots the lanes whose raw resets, commits up to
// the first of them and rescans the lanes behind it from b = 0.  About 7 in 32,761 records reset.
#pragma once
#include <cstdint>

#include "offsets_run.h"  // KVSEP_HD, add_sat, kSkip

namespace kvsep {
namespace logw {

constexpr uint32_t kBlock = 32768;            // db/log_format.h:30
constexpr uint32_t kHeader = 7;               // db/log_format.h:33
constexpr uint32_t kAvail = kBlock - kHeader;  // payload bytes of a fragment that has a block to itself
constexpr uint8_t kFull = 1, kFirst = 2, kMiddle = 3, kLast = 4;  // db/log_format.h:16-24
constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kLayoutThreads = 64;  // the layout kernel: one workgroup of one wavefront
constexpr uint32_t kAhead = 4;           // rows whose len / keep are loaded ahead of the row being resolved
constexpr uint32_t kFillThreads = 256;
constexpr uint64_t kSaturated = offsets::kSaturated;
constexpr uint64_t kSkip = offsets::kSkip;
using offsets::add_sat;

// ---- the writer's offset
KVSEP_HD uint32_t start_state(uint64_t dest_length) { return uint32_t(dest_length % kBlock); }  // log_writer.cc:27-28
// U = b + 7 + len (or its reduced form) -> the raw offset behind the record.  U = 7, an empty record at a block start,
// leaves 7; U = 32768 leaves 32768.
KVSEP_HD uint32_t after(uint32_t u) { return u <= kBlock ? u : 8 + (u - (kBlock + 1)) % kAvail; }
KVSEP_HD bool resets(uint32_t raw) { return raw > kAvail; }  // leftover < 7 (:48): a leftover of exactly 7 holds a header
KVSEP_HD uint32_t pad_bytes(uint32_t raw) { return resets(raw) ? kBlock - raw : 0; }
KVSEP_HD uint32_t start_of(uint32_t raw) { return resets(raw) ? 0 : raw; }

// ---- 32-bit sums.  A value over 32768 is kept as 32769 + (v - 32769) mod 32761, which is congruent to v modulo 32761
// and on the same side of 32768; values up to 32768 stay exact.  The sum of two reduced values is therefore congruent
// to the exact sum and over 32768 exactly when the exact sum is (a term over 32768 stays over it; otherwise nothing was
// reduced), so reducing it again gives reduce(exact sum), and after(reduce(v)) = 8 + (reduce(v) - 32769) mod 32761 =
// 8 + (v - 32769) mod 32761 = after(v) for v > 32768, after(v) itself below.  A reduced value is under 2^16, so 64 of
// them and a start offset fit 32 bits with room to spare.
KVSEP_HD uint32_t reduce(uint64_t v) { return v <= kBlock ? uint32_t(v) : uint32_t(kBlock + 1 + (v - (kBlock + 1)) % kAvail); }
// What a record adds to the running sum: 7 + len, reduced (the header is added to the reduced length, so a length of
// 2^64 - 1 does not wrap); a dropped record adds nothing.
KVSEP_HD uint32_t step_of(bool kept, uint64_t len) { return kept ? reduce(uint64_t(reduce(len)) + kHeader) : 0; }
// The running sum from offset b: b + sum, reduced.
KVSEP_HD uint32_t join(uint32_t b, uint32_t sum) { return reduce(uint64_t(b) + sum); }

// ---- a row of 64 records.  `todo` are the lanes not yet committed, `incl` a lane's inclusive sum of step_of over the
// todo lanes, `r` the raw offset in front of the first todo lane.
KVSEP_HD uint64_t lanes_below(uint32_t lane) { return (uint64_t(1) << lane) - 1; }
KVSEP_HD uint64_t lanes_upto(uint32_t lane) { return lane >= 63 ? ~uint64_t(0) : (uint64_t(1) << (lane + 1)) - 1; }
// The raw offset behind a lane's record, were there no reset among the todo lanes before it.
KVSEP_HD uint32_t row_u(uint32_t r, uint32_t incl) { return after(join(start_of(r), incl)); }
// The raw offset in front of a lane: r itself while no kept todo lane lies before it (a dropped record changes
// nothing, and r may be a reset the first kept record still has to take), else what the lane before left.
KVSEP_HD uint32_t raw_before(uint32_t r, bool kept_before, uint32_t excl) { return kept_before ? row_u(r, excl) : r; }
// The raw offset behind a lane: the same with the lane itself counted (kept_upto, its inclusive sum).  With one record
// in the "row" this is the serial step of kvsep_log_frame_layout.
KVSEP_HD uint32_t raw_behind(uint32_t r, bool kept_upto, uint32_t incl) { return raw_before(r, kept_upto, incl); }
// The lanes one scan step commits: all of todo when no kept todo lane leaves a reset (`reset` = their ballot), else up
// to and including the first that does.  The lanes behind it are scanned again with their sum restarted.
KVSEP_HD uint64_t commit_mask(uint64_t todo, uint64_t reset) {
  return reset ? todo & lanes_upto(uint32_t(__builtin_ctzll(reset))) : todo;
}
KVSEP_HD uint32_t last_lane(uint64_t m) { return 63u - uint32_t(__builtin_clzll(m)); }  // m != 0

// ---- fragments and blocks of a record whose first header goes to offset b <= 32761
KVSEP_HD uint64_t nfrag(uint32_t b, uint64_t len) {
  const uint64_t first = kAvail - b;
  return len <= first ? 1 : 1 + (len - first - 1) / kAvail + 1;  // 1 + ceil((len - first) / 32761)
}
// Blocks between the raw offset in front of the record and the one behind it: every fragment but the first starts one,
// and so does a reset.  A record's position is then block * 32768 + offset; no byte count is summed fragment by fragment.
KVSEP_HD uint64_t blocks_advanced(bool reset, uint64_t nf) { return nf - 1 + (reset ? 1 : 0); }
// block * 32768 + raw, saturating at 2^64 - 1.
KVSEP_HD uint64_t pos_sat(uint64_t block, uint32_t raw) {
  return block > (kSaturated - kBlock) / kBlock ? kSaturated : block * kBlock + raw;
}
// A position relative to the call's first byte (the log's dest_length, at offset b0 of block 0).
KVSEP_HD uint64_t rel(uint64_t pos, uint32_t b0) { return pos == kSaturated ? kSaturated : pos - b0; }
// A record is laid out when it is kept and its end (its blocks' inclusive sum, its raw offset) does not saturate; a
// record that is not owns no fragment and gets kSkip.  The sums are monotone, so every kept record behind a saturated
// one saturates too.
KVSEP_HD bool laid(bool kept, uint64_t block_end, uint32_t raw_end) { return kept && pos_sat(block_end, raw_end) != kSaturated; }
// Where a laid record's first header goes, relative to the call's first byte: its last block less the nf - 1 its
// fragments advanced.
KVSEP_HD uint64_t rec_at(bool is_laid, uint64_t block_end, uint64_t nf, uint32_t b, uint32_t b0) {
  return is_laid ? (block_end - (nf - 1)) * kBlock + b - b0 : kSkip;
}
KVSEP_HD uint64_t frags_of(bool is_laid, uint64_t nf) { return is_laid ? nf : 0; }

// Fragment k < nf of a record of len bytes at offset b: its bytes [frag_begin, + frag_len) of the record, its header at
// frag_at (k >= 1 starts a block), its type.  frag_len <= 32761, so the header's LE16 length holds it.
KVSEP_HD uint64_t frag_begin(uint32_t b, uint64_t k) { return k ? (kAvail - b) + (k - 1) * kAvail : 0; }
KVSEP_HD uint64_t frag_len(uint32_t b, uint64_t len, uint64_t k) {
  const uint64_t room = k ? kAvail : kAvail - b, left = len - frag_begin(b, k);
  return left < room ? left : room;
}
KVSEP_HD uint64_t frag_at(uint64_t at, uint32_t b, uint64_t k) { return k ? at + (k * kBlock - b) : at; }
KVSEP_HD uint8_t frag_type(uint64_t k, uint64_t nf) { return nf == 1 ? kFull : k == 0 ? kFirst : k + 1 == nf ? kLast : kMiddle; }
// The init of a fragment's checksum, Value(&type, 1) (log_writer.cc:16-21), from the four a call was given.
KVSEP_HD uint32_t seed_of(uint8_t type, uint32_t full, uint32_t first, uint32_t middle, uint32_t last) {
  return type == kFull ? full : type == kFirst ? first : type == kMiddle ? middle : last;
}

// The record that owns fragment slot f < frag_first[count]: the last i in [0, count) with frag_first[i] <= f.  Records
// that own no fragment tie with the record behind them, which the search passes over.  `at(i)` reads frag_first[i];
// every index it is called with lies in [0, count) (count != 0).
template <class At>
KVSEP_HD uint64_t owner(uint64_t f, uint64_t count, At at) {
  uint64_t lo = 0, hi = count;  // frag_first[lo] <= f (frag_first[0] = 0), hi is past the answer
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (at(mid) <= f) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- the scratch word of a record (its offset b and its pad count) and the padding of the outputs
KVSEP_HD uint32_t pack_rec(uint32_t b, uint32_t pad) { return b | pad << 16; }
KVSEP_HD uint32_t rec_b(uint32_t w) { return w & 0xffffu; }
KVSEP_HD uint32_t rec_pad(uint32_t w) { return w >> 16; }
// Fragment slots the arrays hold, and whether slot f is padding.
KVSEP_HD uint64_t held(uint64_t nf, uint64_t cap) { return nf < cap ? nf : cap; }
KVSEP_HD bool pads_frag(uint64_t f, uint64_t nf, uint64_t cap) { return f >= nf && f < cap; }
constexpr uint64_t kPadOff = 0, kPadLen = 0, kPadAt = kSkip;
constexpr uint8_t kPadType = 0;
constexpr uint32_t kPadSeed = 0;
// A record's pad zeros [at - pad, at) are written when its first fragment is stored (first_frag < frag_cap) and the
// zeros lie inside [0, dst_bytes).
KVSEP_HD bool writes_pad(uint64_t at, uint32_t pad, uint64_t first_frag, uint64_t frag_cap, uint64_t dst_bytes) {
  return pad != 0 && at != kSkip && pad <= at && first_frag < frag_cap && at <= dst_bytes;
}
// The grids: a lane per fragment slot and per record, whichever are more.
KVSEP_HD uint64_t fill_lanes(uint64_t count, uint64_t frag_cap) { return count > frag_cap ? count : frag_cap; }
KVSEP_HD uint64_t row_count(uint64_t count) { return (count + kWaveLanes - 1) / kWaveLanes; }

}  // namespace logw
}  // namespace kvsep
