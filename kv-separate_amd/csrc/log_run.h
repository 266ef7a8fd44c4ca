// log_run.h -- the rules of the device log / MANIFEST reader (no HIP, no allocation: tests/cpp/log_run_test.cc builds it
// alone and runs the kernels' control flow lane by lane against a plain serial loop).  The kernels (crc32c_logwalk.inc)
// take every decision below from here: a block's extent (block_begin, block_end), what stands at a header position
// (has_header, header_len, classify), where the next header is (next_header), which walked records belong to a block
// (first_in_block, in_block), what a block leaves in `pending` (block_pending, resolve), which records are dead
// (dies), which one stops the reader (stops, stop_min), what each record gets (Verdict, judge) and which byte counts
// are reported (mismatch_bytes, bad_length_bytes, counts_bad_length).
//
// The reader is log::Reader::ReadPhysicalRecord (db/log_reader.cc:189-272), as kvsep_log_walk and
// kvsep_log_accept_gaps (framing.cpp) restate it on the host.  The format is cut into 32 KiB blocks and no physical
// record spans two, so a block is walked on its own.  Three things cross a block's end:
//   the record index    record k of block b is record base[b] + k, base = the exclusive prefix sum of the blocks' counts;
//   `pending`           a reader event without a record (bad length, zero header) since the last live record: gap[i] of
//                       the next live record.  A block with a record below `count` sets it on its own account (kSet /
//                       kClear), a block whose only event is such a skip sets it (kSet), and only a block with neither --
//                       a final block of fewer than 7 bytes -- passes it through (kPass);
//   `stopped`           the first live record with a good checksum and type 5 (kEof): a minimum over the blocks.
#pragma once
#include <cstdint>

#include "concat_run.h"  // KVSEP_HD

namespace kvsep {
namespace logrun {

constexpr uint64_t kBlock = 32768;  // db/log_format.h:30
constexpr uint64_t kHeader = 7;     // db/log_format.h:33
constexpr uint64_t kTypeAt = 6;     // off[i] = header + 6: the CRC covers type || payload (log_reader.cc:247-248)
constexpr uint8_t kEofCode = 5;     // db/log_reader.h:66: kEof = kMaxRecordType + 1 ...
constexpr uint8_t kBadCode = 6;     // ... :72 kBadRecord = + 2, in the value space of the type byte
constexpr uint64_t kNone = ~uint64_t(0);  // no stop
constexpr uint32_t kThreads = 256;  // lanes per workgroup of the block kernels: a lane owns a block
constexpr uint32_t kPadPerLane = 16;  // padding elements a lane of the fill / accept kernel is sized for

// ---- blocks
KVSEP_HD uint64_t block_count(uint64_t n) { return n / kBlock + (n % kBlock ? 1 : 0); }
KVSEP_HD uint64_t block_begin(uint64_t blk) { return blk * kBlock; }
KVSEP_HD uint64_t block_end(uint64_t blk, uint64_t n) { return n - blk * kBlock > kBlock ? (blk + 1) * kBlock : n; }
KVSEP_HD bool block_full(uint64_t begin, uint64_t end) { return end - begin == kBlock; }
KVSEP_HD uint64_t grid_for(uint64_t items) { return (items + kThreads - 1) / kThreads; }
constexpr uint32_t kReduceGrid = 1;  // log_stop_kernel and log_totals_kernel: one workgroup strides over the blocks
// The grid of the two kernels whose lanes walk a block each and then share out the padding from min(*nrec, cap) to
// cap, lane g taking elements g, g + lanes, ...: a lane per block, about kPadPerLane elements a lane, one workgroup at
// least (an empty image still has its padding and its words to write).
KVSEP_HD uint64_t pad_grid(uint64_t nblocks, uint64_t cap) {
  const uint64_t pad = (cap + kPadPerLane - 1) / kPadPerLane;
  const uint64_t items = nblocks > pad ? nblocks : pad;
  return grid_for(items ? items : 1);
}

// The reader's scratch words, one array: the stop index, then kLogWords per block -- its record count, the records
// before it, its first record, `pending` state, stop candidate, dropped bytes and bad-length bytes.  A call over nblocks
// blocks slices it at words(nblocks); an array that holds nblocks blocks has scratch_words(nblocks) words.
constexpr uint64_t kStopWords = 1;
constexpr uint64_t kLogWords = 7;
struct Words {
  uint64_t stop, cnt, base, first, state, cand, drop, badlen;
};
KVSEP_HD Words words(uint64_t nblocks) {
  const uint64_t w = kStopWords, nb = nblocks;
  return {0, w, w + nb, w + 2 * nb, w + 3 * nb, w + 4 * nb, w + 5 * nb, w + 6 * nb};
}
KVSEP_HD uint64_t scratch_words(uint64_t nblocks) { return kStopWords + kLogWords * nblocks; }

// ---- headers
enum Head : uint32_t { kRecord = 0, kBadLength = 1, kZero = 2, kTrailer = 3 };

// Fewer than 7 bytes left in the block: a trailer, and the header is not read (:192-215).
KVSEP_HD bool has_header(uint64_t p, uint64_t end) { return end - p >= kHeader; }
KVSEP_HD uint64_t header_len(uint8_t b4, uint8_t b5) { return uint64_t(b4) | (uint64_t(b5) << 8); }
KVSEP_HD uint32_t header_stored(uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3) {
  return uint32_t(b0) | (uint32_t(b1) << 8) | (uint32_t(b2) << 16) | (uint32_t(b3) << 24);
}
// What the header at p (has_header) is: a length past the block end (:224-235), a preallocated zero header (:237-243),
// else a physical record.
KVSEP_HD Head classify(uint64_t p, uint64_t end, uint64_t l, uint8_t t) {
  if (kHeader + l > end - p) return kBadLength;
  if (t == 0 && l == 0) return kZero;
  return kRecord;
}
KVSEP_HD bool is_skip(Head h) { return h == kBadLength || h == kZero; }
KVSEP_HD uint64_t next_header(uint64_t p, uint64_t l) { return p + kHeader + l; }
KVSEP_HD uint64_t rec_off(uint64_t p) { return p + kTypeAt; }
KVSEP_HD uint64_t rec_len(uint64_t l) { return 1 + l; }

// ---- the walked arrays, per block
// How many of the arrays' elements hold records: the walk's count cut to the arrays' capacity.
KVSEP_HD uint64_t held(uint64_t nrec, uint64_t cap) { return nrec < cap ? nrec : cap; }
// The lower bound a block's lane searches off[0, held) for: its first record is the first i with off[i] >= this.
KVSEP_HD uint64_t first_in_block(uint64_t begin) { return begin + kTypeAt; }
// One step of that search over [lo, hi): the probe index, and which half remains.
KVSEP_HD uint64_t probe(uint64_t lo, uint64_t hi) { return lo + (hi - lo) / 2; }
KVSEP_HD bool probe_right(uint64_t off_mid, uint64_t want) { return off_mid < want; }
// Does record off (>= first_in_block(begin) by the search) lie in the block: its header fits before the end.
KVSEP_HD bool in_block(uint64_t off, uint64_t begin, uint64_t end) {
  return off >= begin + kTypeAt && off < end;  // off < end: the 7 bytes from off - 6 lie before the end
}
KVSEP_HD uint64_t header_of(uint64_t off) { return off - kTypeAt; }
// Where the header after record (off, len) stands, never past the block's end whatever the arrays say.
KVSEP_HD uint64_t after_record(uint64_t off, uint64_t len, uint64_t end) {
  return len > end - off ? end : off + len;
}

// ---- the accept rule
// A live record with a bad checksum drops the rest of its block buffer: it and every later record of the block are dead.
KVSEP_HD bool dies(bool dead, uint8_t ok) { return dead || !ok; }
// A live record with a good checksum and type 5 reads as kEof: nothing after it is read (:270-271).
KVSEP_HD bool stops(bool dead, uint8_t ok, uint8_t t) { return !dead && ok && t == kEofCode; }
KVSEP_HD uint64_t stop_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// What a block leaves in `pending`.
enum Pending : uint32_t { kPass = 0, kClear = 1, kSet = 2 };
// any = the block holds a record below `count`; dead = one of them failed its checksum; tail = what stands where the
// block's records end.  A skip the reader reaches sets it; else the block's first record cleared it.
KVSEP_HD Pending block_pending(bool any, bool dead, Head tail) {
  if (is_skip(tail) && !dead) return kSet;
  return any ? kClear : kPass;
}
// `pending` on entry to a block from the state of the block before it: true when decided (then *pending holds it), false
// to look one block further back.  Before block 0 nothing is pending.
KVSEP_HD bool resolve(Pending before, bool* pending) {
  *pending = before == kSet;
  return before != kPass;
}

// The bytes reported with "bad record length": only while eof_ is unset, i.e. when the block was read in full
// (:227-235), and only where the reader gets that far (not in a dead block).
KVSEP_HD uint64_t bad_length_bytes(Head tail, bool dead, uint64_t begin, uint64_t end, uint64_t p) {
  return tail == kBadLength && !dead && block_full(begin, end) ? end - p : 0;
}
// ... and only in blocks before the one that holds the stop: [lo, hi) = the block's record indices, stop = the stop
// index.  A block with stop < hi holds the stop or lies after it: the reader never gets to its end.
// (kNone is the largest index, so it is past every block.)
KVSEP_HD bool counts_bad_length(uint64_t hi, uint64_t stop) { return stop >= hi; }
// The bytes reported with "checksum mismatch": the bad record's header to the end of its block buffer (:255-257).
KVSEP_HD uint64_t mismatch_bytes(uint64_t header, uint64_t end) { return end - header; }

struct Verdict {
  uint8_t accept, gap;
  bool dead;      // the block is dead from here on
  bool mismatch;  // this record is the one that killed it
};
// Record i: dead = the block was dropped before it, pending = the carried value, stop = the stop index.
KVSEP_HD Verdict judge(uint64_t i, uint64_t stop, bool dead, bool pending, uint8_t ok, uint8_t t) {
  if (i > stop || dead) return {0, 0, dead, false};  // never read (stop == kNone: no i is past it)
  const uint8_t gap = pending ? 1 : 0;
  if (!ok) return {0, gap, true, true};
  if (t == kEofCode) return {0, gap, false, false};
  return {uint8_t(t == kBadCode ? 0 : 1), gap, false, false};
}

}  // namespace logrun
}  // namespace kvsep
