// sstw_run.h -- the rules of the SST table writer: index block build, metaindex block, footer (no HIP, no allocation:
// tests/cpp/sstw_run_test.cc builds it alone and runs the kernels' control flow lane by lane against a serially restated
// BlockBuilder and Footer::EncodeTo).  The kernels (crc32c_sstbuild.inc) and the host forms (framing.cpp:
// kvsep_sst_index_build, kvsep_sst_footer_build) take every decision below from here.
//
// The format is the reference's: BlockBuilder::Add / Finish (table/block_builder.cc) at block_restart_interval = 1,
// which is how TableBuilder writes index blocks (table/table_builder.cc:36,92), so every entry is a restart point and
// stores its key whole:
//   entry    varint32(shared = 0) varint32(key_len) varint32(value_len) key varint64(off) varint64(len)
//   block    the kept entries in order, restart[k] = byte position of the k-th kept entry (LE32), the restart count
//   empty    no kept entry: one restart of 0 and a count of 1, 8 bytes (BlockBuilder's restarts_ starts as {0})
//   trailer  [type 0][Mask(Extend(Value(block), "\0", 1)) LE32]   (table/table_builder.cc:209-232)
//   footer   varint64 x 4 (metaindex handle, index handle), zeros to 40 bytes, the magic LE64 (table/format.cc:23-35)
#pragma once
#include <cstdint>

#include "concat_run.h"  // KVSEP_HD
#include "sst_run.h"     // the source status codes

namespace kvsep {
namespace sstw {

// ---- status codes (KVSEP_SSTW_* of the public header)
constexpr uint32_t kOk = 0, kTooLarge = 1, kNoRoom = 2, kSource = 3;

constexpr uint64_t kSaturated = ~uint64_t(0);
constexpr uint64_t kSkip = ~uint64_t(0);            // blk_off of a block that was not laid out (offsets::kSkip)
constexpr uint64_t kTrailer = 5;                    // table/format.h: kBlockTrailerSize
constexpr uint64_t kFooter = 48;                    // table/format.h: Footer::kEncodedLength
constexpr uint64_t kMagic = 0xdb4775248b80fb57ull;  // table/format.h: kTableMagicNumber
constexpr uint64_t kEmptyBlock = 8;                 // one restart of 0, a count of 1
constexpr uint64_t kMetaFramed = kEmptyBlock + kTrailer;  // the table form's metaindex block with its trailer
constexpr uint64_t kMaxBlock = 0xffffffffull;       // restart offsets are 32-bit: a block stays below 2^32 bytes
constexpr uint64_t kMaxKey = 0xffffffffull;         // non_shared is a varint32
constexpr uint32_t kThreads = 256;                  // lanes per workgroup: a lane owns an entry
constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kWaves = kThreads / kWaveLanes;
constexpr uint32_t kGran = 16;                      // the aligned store of the fill
constexpr uint32_t kTailThreads = 64;               // sstw_tail_kernel: one wavefront
// The staging threshold: a wavefront whose 64 entries encode to at most this many bytes stages them in LDS and stores
// the range in 16-B granules; a longer range (one key over the threshold is enough) is written entry by entry by the
// whole wave, straight to the destination.  64 entries of a 16-byte user key and its 8-byte tag take about 2 KiB.
constexpr uint32_t kStageBytes = 4096;
constexpr uint32_t kStageGranules = kStageBytes / kGran + 1;  // the range starts at its destination's phase in [0, 16)

KVSEP_HD uint64_t add_sat(uint64_t a, uint64_t b) { return a + b < a ? kSaturated : a + b; }
KVSEP_HD uint64_t grid_for(uint64_t count) { return count ? (count + kThreads - 1) / kThreads : 1; }

// ---- scratch: per entry its size, its kept flag, its byte position and its rank among the kept (four u64 arrays), a
// keep byte per entry for the rewrite (rounded up to words), then the builder's words.
enum Word : uint64_t { kEntriesBytes = 0, kNKept, kCrcOff, kCrcLen, kCrc, kDataEnd, kSalvaged, kWords = 8 };
struct Slices {
  uint64_t size, flag, pos, rank, keep, words;
};
KVSEP_HD Slices slices(uint64_t count) {
  return {0, count, 2 * count, 3 * count, 4 * count, 4 * count + (count + 7) / 8};
}
KVSEP_HD uint64_t scratch_words(uint64_t count) { return slices(count).words + kWords; }

// ---- varints (util/coding.cc)
KVSEP_HD uint32_t varint_len(uint64_t v) {
  uint32_t n = 1;
  for (; v >= 128; v >>= 7) ++n;
  return n;
}
// Byte k < varint_len(v) of v's encoding.
KVSEP_HD uint8_t varint_byte(uint64_t v, uint32_t k) {
  const uint64_t r = v >> (7 * k);
  return uint8_t((r & 127) | (r >= 128 ? 128 : 0));
}

// ---- the three decisions tests/cpp/sstw_run_test.cc swaps for wrong ones, to show that it would notice
struct Rule {
  // The restart array has an entry per kept entry, and one (of 0) when there is none.
  static KVSEP_HD uint64_t restarts(uint64_t nkept) { return nkept ? nkept : 1; }
  // A kept entry's restart slot is its rank among the kept, not its index.
  static KVSEP_HD uint64_t slot(uint64_t rank, uint64_t /*index*/) { return rank; }
  // The granule stores of a range begin at the first 16-B boundary at or after its first byte.
  static KVSEP_HD uint64_t body_begin(uint64_t d) { return (d + kGran - 1) & ~uint64_t(kGran - 1); }
};

// ---- the keep rule: the salvage's ok[] and dst_off[] go in as they are.  mask = keep[i] (1 without a keep array).
KVSEP_HD bool kept(uint8_t mask, uint64_t blk_off) { return mask != 0 && blk_off != kSkip; }

// ---- an entry
KVSEP_HD uint32_t value_len(uint64_t off, uint64_t len) { return varint_len(off) + varint_len(len); }  // <= 20: a byte
KVSEP_HD uint32_t head_len(uint64_t key_len) { return 2 + varint_len(key_len); }
// The encoded size: 0 when dropped, saturated when the key is longer than a varint32 holds.
KVSEP_HD uint64_t entry_size(bool keep, uint64_t key_len, uint64_t off, uint64_t len) {
  if (!keep) return 0;
  if (key_len > kMaxKey) return kSaturated;
  return head_len(key_len) + key_len + value_len(off, len);
}
// Byte j < head_len of the three header varints.
KVSEP_HD uint8_t head_byte(uint32_t j, uint64_t key_len, uint32_t vlen) {
  if (j == 0) return 0;
  return j + 1 < head_len(key_len) ? varint_byte(key_len, j - 1) : uint8_t(vlen);
}
// Byte j < value_len of the handle.
KVSEP_HD uint8_t value_byte(uint32_t j, uint64_t off, uint64_t len) {
  const uint32_t n = varint_len(off);
  return j < n ? varint_byte(off, j) : varint_byte(len, j - n);
}
// Byte j of a whole entry that is not a key byte: j < head_len, or j >= head_len + key_len.
KVSEP_HD uint8_t frame_byte(uint64_t j, uint64_t key_len, uint64_t off, uint64_t len) {
  const uint32_t h = head_len(key_len);
  return j < h ? head_byte(uint32_t(j), key_len, value_len(off, len)) : value_byte(uint32_t(j - h - key_len), off, len);
}

// ---- the block
template <class R = Rule>
KVSEP_HD uint64_t block_len(uint64_t entries_bytes, uint64_t nkept) {
  return add_sat(entries_bytes, 4 * R::restarts(nkept) + 4);  // nkept < 2^32: the product cannot wrap
}
template <class R = Rule>
KVSEP_HD uint64_t restart_at(uint64_t entries_bytes, uint64_t rank, uint64_t index) {
  return entries_bytes + 4 * R::slot(rank, index);
}
template <class R = Rule>
KVSEP_HD uint64_t count_at(uint64_t entries_bytes, uint64_t nkept) { return entries_bytes + 4 * R::restarts(nkept); }
template <class R = Rule>
KVSEP_HD uint32_t count_word(uint64_t nkept) { return uint32_t(R::restarts(nkept)); }
// Does the block have a restart that no entry writes (the empty block's one restart of 0)?
template <class R = Rule>
KVSEP_HD bool lone_restart(uint64_t nkept) { return nkept == 0 && R::restarts(nkept) != 0; }

// The source statuses (KVSEP_SST_*) after which a rewrite writes nothing: a bad footer, an index block that failed its
// check or is compressed, and prefix-compressed keys, which this form does not expand.
KVSEP_HD bool refuses(uint32_t source_status) {
  return source_status == sst::kBadFooter || source_status == sst::kIndexChecksum ||
         source_status == sst::kIndexCompressed || source_status == sst::kSharedKey;
}

struct Plan {
  uint32_t status;
  uint64_t len;   // the block's bytes that are written: 0 after a refusal
  uint64_t need;  // the block's length as it would be: 0 when too large or when the source refuses
  uint64_t at;    // where the block starts: the caller's position plus `lead`
};
// The refusals, from the totals: `lead` bytes go before the block (the table form's metaindex block) and `trail` after
// its trailer (the footer).  Formed with no sum that can wrap: lead + len + 5 + trail < 2^33.
template <class R = Rule>
KVSEP_HD Plan plan(uint64_t entries_bytes, uint64_t nkept, uint64_t at, uint64_t lead, uint64_t trail,
                   uint64_t dst_bytes, uint32_t source_status) {
  if (refuses(source_status)) return {kSource, 0, 0, 0};
  const uint64_t len = block_len<R>(entries_bytes, nkept);
  if (len > kMaxBlock) return {kTooLarge, 0, 0, 0};
  if (at > dst_bytes || lead + len + kTrailer + trail > dst_bytes - at) return {kNoRoom, 0, len, 0};
  return {kOk, len, len, at + lead};
}
// What the table form reports as *table_bytes.
KVSEP_HD uint64_t table_bytes(const Plan& p) { return p.status ? 0 : p.at + p.len + kTrailer + kFooter; }

// ---- the fill: a wavefront's entries are the bytes [w0, w1) of the block
KVSEP_HD bool stages(uint64_t range_bytes) { return range_bytes <= kStageBytes; }
// A range of n >= 1 bytes at destination address d: bytes [0, head) and [n - tail, n) are byte stores, the `body`
// granules between are naturally aligned 16-B stores.
struct Span {
  uint64_t head, body, tail;
};
template <class R = Rule>
KVSEP_HD Span split(uint64_t d, uint64_t n) {
  const uint64_t b0 = R::body_begin(d), e = d + n;
  const uint64_t b1 = e & ~uint64_t(kGran - 1);
  if (b0 >= b1) return {n, 0, 0};
  return {b0 - d, (b1 - b0) / kGran, e - b1};
}
// Edge byte k < head + tail of the span: its index in the range.
KVSEP_HD uint64_t edge_index(const Span& s, uint64_t n, uint64_t k) { return k < s.head ? k : n - s.tail + (k - s.head); }

// ---- the trailer, the metaindex block, the footer
KVSEP_HD uint8_t trailer_byte(uint32_t j, uint32_t masked) { return j == 0 ? 0 : uint8_t(masked >> (8 * (j - 1))); }
// Byte j < 13 of the empty block with its trailer; masked = Mask(Value of the 8 bytes and the type byte).
KVSEP_HD uint8_t meta_byte(uint32_t j, uint32_t masked) {
  if (j < kEmptyBlock) return j == 4 ? 1 : 0;
  return trailer_byte(j - uint32_t(kEmptyBlock), masked);
}
KVSEP_HD uint8_t footer_byte(uint32_t j, uint64_t moff, uint64_t mlen, uint64_t ioff, uint64_t ilen) {
  if (j >= 40) return uint8_t(kMagic >> (8 * (j - 40)));
  uint32_t n = varint_len(moff);
  if (j < n) return varint_byte(moff, j);
  j -= n;
  n = varint_len(mlen);
  if (j < n) return varint_byte(mlen, j);
  j -= n;
  n = varint_len(ioff);
  if (j < n) return varint_byte(ioff, j);
  j -= n;
  n = varint_len(ilen);
  return j < n ? varint_byte(ilen, j) : 0;
}

}  // namespace sstw
}  // namespace kvsep
