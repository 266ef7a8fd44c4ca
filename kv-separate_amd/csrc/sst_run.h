// sst_run.h -- the rules of the SST table reader: footer, index-block walk, slot layout of the table form (no HIP, no
// allocation: tests/cpp/sst_run_test.cc builds it alone and runs the kernels' control flow lane by lane against a plain
// serial loop).  The kernels (crc32c_sstindex.inc) and the host forms (framing.cpp: kvsep_sst_footer,
// kvsep_sst_index_walk) take every decision below from here; all they add is where a byte comes from (the `Rd` of the
// templates: rd(p) = byte p of the image) and where a handle goes (the `Emit`).
//
// The format is the reference's: Footer::DecodeFrom (table/format.cc:37-60), Block::Block and DecodeEntry
// (table/block.cc:27-82), BlockHandle::DecodeFrom, the restart array of BlockBuilder (table/block_builder.cc).  An
// index block ends in its restart array, and an entry at a restart point shares nothing with the entry before it, so a
// restart run is walked on its own.  Two things cross a run's end:
//   the entry index   entry k of run r is entry base[r] + k, base = the exclusive prefix sum of the runs' counts;
//   the stop          the lowest run with an error: nothing of a later run is emitted.
// On a block with no error the emitted handles are what Block::Iter yields from SeekToFirst to the end.  Where the
// rules are stricter than that iterator (which never looks at the restart array while it steps), the block has an
// error here: a restart array that is not strictly increasing from 0 below restart_offset, an entry at a restart point
// that shares key bytes, an entry that crosses a restart point.
#pragma once
#include <cstdint>

#include "concat_run.h"  // KVSEP_HD

namespace kvsep {
namespace sst {

// ---- status codes (KVSEP_SST_* of the public header)
constexpr uint32_t kOk = 0, kBadFooter = 1, kIndexChecksum = 2, kIndexCompressed = 3, kBadRestarts = 4, kBadEntry = 5,
                   kBadHandle = 6, kCap = 7, kSharedKey = 8;

constexpr uint64_t kFooter = 48;                     // table/format.h: Footer::kEncodedLength
constexpr uint64_t kMagicBytes = 8;
constexpr uint64_t kMagic = 0xdb4775248b80fb57ull;   // table/format.h: kTableMagicNumber
constexpr uint64_t kTrailer = 5;                     // table/format.h: kBlockTrailerSize
constexpr uint64_t kNone = ~uint64_t(0);             // no run has an error
constexpr uint64_t kSkip = ~uint64_t(0);             // base[r] of a run past the stop (offsets::kSkip)
constexpr uint32_t kThreads = 256;                   // lanes per workgroup of the run kernels: a lane owns a run
constexpr uint32_t kPadPerLane = 16;                 // padding elements a lane of the fill kernel is sized for
constexpr uint32_t kFooterThreads = 64;              // sst_footer_kernel: one wavefront, lane 0 decodes
constexpr uint32_t kMaskOfZero = 0xa282ead8u;        // Mask(0): the stored word a block of length 0 matches
constexpr uint32_t kNoMatch = ~kMaskOfZero;          // ... and one it cannot match

// ---- scratch and grids
KVSEP_HD uint64_t grid_for(uint64_t items) { return (items + kThreads - 1) / kThreads; }
// Scratch words of a walk over at most `runs` restart runs: the keep_before word and the stop's error word, then per
// run its count and one more word that first holds its error (until the stop kernel has read it) and then its base,
// then per workgroup of the count kernel the lowest of its runs that has an error.
constexpr uint64_t kStopWords = 2;
KVSEP_HD uint64_t scratch_words(uint64_t runs) { return kStopWords + 2 * runs + grid_for(runs); }
// The runs kvsep_crc32c_reserve(ctx, count, ...) sizes for, and the runs a call gets: what is reserved, cap when that
// is more (an eager call may allocate), one at least (lane 0 reports a block that has no run at all).
KVSEP_HD uint64_t runs_reserved(uint64_t count) { return count; }
KVSEP_HD uint64_t runs_for(uint64_t reserved, uint64_t cap) {
  const uint64_t r = reserved > cap ? reserved : cap;
  return r ? r : 1;
}
// The runs one call launches lanes for: what the scratch holds, but no more than an image of n bytes can hold (a
// restart is 4 bytes), so a large reservation does not make a small table's walk large.
KVSEP_HD uint64_t runs_used(uint64_t held_by_scratch, uint64_t n) {
  const uint64_t most = n / 4 ? n / 4 : 1;
  return held_by_scratch < most ? held_by_scratch : most;
}
// The fill kernel: a lane per run, and about kPadPerLane padding elements a lane.
KVSEP_HD uint64_t pad_grid(uint64_t runs, uint64_t cap) {
  const uint64_t pad = (cap + kPadPerLane - 1) / kPadPerLane;
  const uint64_t items = runs > pad ? runs : pad;
  return grid_for(items ? items : 1);
}

// ---- the three decisions tests/cpp/sst_run_test.cc swaps for wrong ones, to show that it would notice
struct Rule {
  // Do the `need` key-delta and value bytes at p lie inside the run that ends at `end`?  (restart_offset: the end of
  // the block's entries, which a wrong rule might take instead.)
  static KVSEP_HD bool fits(uint64_t need, uint64_t p, uint64_t end, uint64_t /*restart_offset*/) {
    return need <= end - p;
  }
  // The first entry of a run has nothing before it to share with.
  static KVSEP_HD bool first_shared_ok(uint32_t shared) { return shared == 0; }
  // Of two runs with an error the lower one stops the walk.
  static KVSEP_HD uint64_t stop_pick(uint64_t a, uint64_t b) { return a < b ? a : b; }
};

// ---- bytes
template <class Rd>
KVSEP_HD uint32_t le32(Rd& rd, uint64_t p) {
  return uint32_t(rd(p)) | (uint32_t(rd(p + 1)) << 8) | (uint32_t(rd(p + 2)) << 16) | (uint32_t(rd(p + 3)) << 24);
}
template <class Rd>
KVSEP_HD uint64_t le64(Rd& rd, uint64_t p) {
  return uint64_t(le32(rd, p)) | (uint64_t(le32(rd, p + 4)) << 32);
}

struct Var {
  uint64_t v, next;
  bool ok;
};
// A varint of at most kBits payload bits in [p, limit): 5 bytes for 32 bits, 10 for 64 (util/coding.cc); a byte at or
// past limit is not read.
template <uint32_t kBits, class Rd>
KVSEP_HD Var varint(Rd& rd, uint64_t p, uint64_t limit) {
  uint64_t v = 0;
  for (uint32_t shift = 0; shift < kBits && p < limit; shift += 7) {
    const uint64_t b = rd(p++);
    v |= (b & 127) << shift;
    if (!(b & 128)) return {kBits == 32 ? uint64_t(uint32_t(v)) : v, p, true};
  }
  return {0, p, false};
}

// ---- handles
// May (off, len) be dereferenced in an image of n bytes: the block and its 5-byte trailer lie inside.  No sum wraps.
KVSEP_HD bool usable(uint64_t off, uint64_t len, uint64_t n) {
  return off <= n && len <= n - off && n - off - len >= kTrailer;
}

// ---- the footer
struct Footer {
  uint64_t h[4];  // meta_off, meta_len, index_off, index_len; all 0 unless status == kOk
  uint32_t status;
};
template <class Rd>
KVSEP_HD Footer footer(Rd& rd, uint64_t n) {
  const Footer bad{{0, 0, 0, 0}, kBadFooter};
  if (n < kFooter) return bad;
  if (le64(rd, n - kMagicBytes) != kMagic) return bad;
  Footer f{{0, 0, 0, 0}, kOk};
  uint64_t p = n - kFooter;
  for (int k = 0; k < 4; ++k) {
    const Var v = varint<64>(rd, p, n - kMagicBytes);
    if (!v.ok) return bad;
    f.h[k] = v.v;
    p = v.next;
  }
  if (!usable(f.h[0], f.h[1], n) || !usable(f.h[2], f.h[3], n)) return bad;
  return f;
}

// ---- the block tail
struct Tail {
  uint64_t nrestarts, restart_offset;
  bool ok;
};
// The block is [base, base + len) of the image.
template <class Rd>
KVSEP_HD Tail tail(Rd& rd, uint64_t base, uint64_t len) {
  if (len < 4) return {0, 0, false};
  const uint64_t nr = le32(rd, base + len - 4);
  if (nr > (len - 4) / 4) return {0, 0, false};
  return {nr, len - 4 * (1 + nr), true};
}

// restart[r] after restart[r - 1]: strictly above it, and below the restart array.
KVSEP_HD bool restart_ok(uint64_t prev, uint64_t cur, uint64_t restart_offset) {
  return cur > prev && cur < restart_offset;
}

struct Run {
  uint64_t begin, end;  // block-relative
  bool ok;              // false: restart[r] itself is bad
};
// Run r < nrestarts.  restart[0] must be 0 (then an empty block's one run is [0, 0): no entry, no error).  A run whose
// next restart is bad has no end of its own and is walked to restart_offset; the next run then holds the error.
template <class Rd>
KVSEP_HD Run run_of(Rd& rd, uint64_t base, const Tail& t, uint64_t r) {
  const uint64_t at = base + t.restart_offset;
  const uint64_t b = le32(rd, at + 4 * r);
  const bool ok = r == 0 ? b == 0 : restart_ok(le32(rd, at + 4 * (r - 1)), b, t.restart_offset);
  if (!ok) return {0, 0, false};
  uint64_t e = t.restart_offset;
  if (r + 1 < t.nrestarts) {
    const uint64_t nx = le32(rd, at + 4 * (r + 1));
    if (restart_ok(b, nx, t.restart_offset)) e = nx;
  }
  return {b, e, true};
}

// ---- entries
struct Entry {
  uint32_t status;
  uint64_t next;     // block-relative offset of the entry after this one
  uint64_t key_len;  // shared + non_shared
  uint64_t off, len; // the handle in the value
  uint64_t shared;   // key bytes taken from the entry before: 0 when the key is stored whole
  uint64_t key_at;   // block-relative offset of the non_shared key bytes the entry stores (the whole key when shared == 0)
};
// The entry at block-relative p of a run that ends at `end` (p < end).  first: the run's first entry; prev_key: the key
// length of the entry before it.  Keys are skipped, never read: key_at is the position the decode steps over.
template <class R = Rule, class Rd>
KVSEP_HD Entry entry(Rd& rd, uint64_t base, uint64_t p, uint64_t end, uint64_t restart_offset, bool first,
                     uint64_t prev_key) {
  const Entry bad{kBadEntry, 0, 0, 0, 0, 0, 0};
  if (end - p < 3) return bad;
  uint32_t f[3] = {rd(base + p), rd(base + p + 1), rd(base + p + 2)};
  uint64_t q = p + 3;
  if ((f[0] | f[1] | f[2]) >= 128) {  // not the one-byte fast path: three varint32
    q = p;
    for (int k = 0; k < 3; ++k) {
      const Var v = varint<32>(rd, base + q, base + end);
      if (!v.ok) return bad;
      f[k] = uint32_t(v.v);
      q = v.next - base;
    }
  }
  const uint64_t shared = f[0], non_shared = f[1], value_len = f[2];
  if (first ? !R::first_shared_ok(f[0]) : shared > prev_key) return bad;
  if (!R::fits(non_shared + value_len, q, end, restart_offset)) return bad;
  const uint64_t vp = base + q + non_shared, vend = vp + value_len;
  const Var o = varint<64>(rd, vp, vend);
  if (!o.ok) return {kBadHandle, 0, 0, 0, 0, 0, 0};
  const Var l = varint<64>(rd, o.next, vend);
  if (!l.ok) return {kBadHandle, 0, 0, 0, 0, 0, 0};
  return {kOk, q + non_shared + value_len, shared + non_shared, o.v, l.v, shared, q};
}

struct Walked {
  uint64_t count;   // entries before the run's end or its first error
  uint32_t status;  // that error
};
// The keys walk's extra rule.  Only a key stored whole has a contiguous place in the block: an entry with shared != 0 is
// an error of its own, kSharedKey, under the same first-error rule (the reference writes index blocks at
// block_restart_interval = 1, where shared is always 0).
KVSEP_HD uint32_t key_status(const Entry& e) { return e.shared ? kSharedKey : kOk; }
// One run, one loop for both walks: emit(k, off, len, key_at, key_len) for its k-th good entry; emit returns false to
// end the walk early (nothing more to store).  kKeys: the keys walk, which also stops at key_status.
template <bool kKeys, class R = Rule, class Rd, class Emit>
KVSEP_HD Walked walk_run_as(Rd& rd, uint64_t base, const Run& run, uint64_t restart_offset, Emit&& emit) {
  uint64_t p = run.begin, k = 0, key = 0;
  while (p < run.end) {
    const Entry e = entry<R>(rd, base, p, run.end, restart_offset, k == 0, key);
    if (e.status) return {k, e.status};
    if (kKeys && key_status(e)) return {k, key_status(e)};
    if (!emit(k, e.off, e.len, e.key_at, e.key_len)) return {k + 1, kOk};
    ++k;
    p = e.next;
    key = e.key_len;
  }
  return {k, kOk};
}
// The plain walk: emit(k, off, len).
template <class R = Rule, class Rd, class Emit>
KVSEP_HD Walked walk_run(Rd& rd, uint64_t base, const Run& run, uint64_t restart_offset, Emit&& emit) {
  return walk_run_as<false, R>(rd, base, run, restart_offset,
                               [&](uint64_t k, uint64_t o, uint64_t l, uint64_t, uint64_t) { return emit(k, o, l); });
}
// The keys walk: emit(k, off, len, key_at, key_len) also gets where the entry's key bytes lie in the block.
template <class R = Rule, class Rd, class Emit>
KVSEP_HD Walked walk_run_keys(Rd& rd, uint64_t base, const Run& run, uint64_t restart_offset, Emit&& emit) {
  return walk_run_as<true, R>(rd, base, run, restart_offset, emit);
}

// ---- the count pass
// A run's error word: its code; an error of the whole block (no run of it is walked) is posted by lane 0 with kWhole.
constexpr uint64_t kWhole = 0x100;
KVSEP_HD uint32_t code_of(uint64_t err) { return uint32_t(err & 0xff); }

// What is wrong with the index block as a whole, before any run: `pre` (the table form's verdict on it: kOk,
// kBadFooter, kIndexChecksum or kIndexCompressed), a handle that leaves the image, a bad tail, more runs than the
// scratch holds.  *t is the tail when the answer is kOk.
template <class Rd>
KVSEP_HD uint32_t block_error(Rd& rd, uint64_t n, uint64_t ioff, uint64_t ilen, uint32_t pre, uint64_t runs, Tail* t) {
  *t = Tail{0, 0, false};
  if (pre) return pre;
  if (!usable(ioff, ilen, n)) return kBadFooter;
  *t = tail(rd, ioff, ilen);
  return t->ok && t->nrestarts <= runs ? kOk : kBadRestarts;
}

// The table form's verdict on the index block from its read check: footer status, computed and stored checksum words
// (the stored one masked), the type byte.  The checksum comes first, as in ReadBlock (table/format.cc:99-125).
KVSEP_HD uint32_t gate(uint32_t footer_status, uint32_t crc, uint32_t stored_unmasked, uint8_t type) {
  if (footer_status) return footer_status;
  if (crc != stored_unmasked) return kIndexChecksum;
  return type ? kIndexCompressed : kOk;
}
KVSEP_HD uint32_t unmask(uint32_t m) {
  const uint32_t rot = m - kMaskOfZero;
  return (rot >> 17) | (rot << 15);
}

struct Counted {
  uint64_t cnt, err;
};
// Lane r of `runs` lanes, of either walk.
template <bool kKeys, class R = Rule, class Rd>
KVSEP_HD Counted count_lane_as(Rd& rd, uint64_t n, uint64_t ioff, uint64_t ilen, uint32_t pre, uint64_t runs,
                               uint64_t r) {
  Tail t;
  const uint32_t whole = block_error(rd, n, ioff, ilen, pre, runs, &t);
  if (whole) return {0, r == 0 ? (whole | kWhole) : 0};
  if (r >= t.nrestarts) return {0, 0};
  const Run run = run_of(rd, ioff, t, r);
  if (!run.ok) return {0, kBadRestarts};
  const Walked w = walk_run_as<kKeys, R>(rd, ioff, run, t.restart_offset,
                                         [](uint64_t, uint64_t, uint64_t, uint64_t, uint64_t) { return true; });
  return {w.count, w.status};
}
template <class R = Rule, class Rd>
KVSEP_HD Counted count_lane(Rd& rd, uint64_t n, uint64_t ioff, uint64_t ilen, uint32_t pre, uint64_t runs,
                            uint64_t r) {
  return count_lane_as<false, R>(rd, n, ioff, ilen, pre, runs, r);
}
template <class R = Rule, class Rd>
KVSEP_HD Counted count_lane_keys(Rd& rd, uint64_t n, uint64_t ioff, uint64_t ilen, uint32_t pre, uint64_t runs,
                                 uint64_t r) {
  return count_lane_as<true, R>(rd, n, ioff, ilen, pre, runs, r);
}

// ---- the stop
// A lane's candidate: its run when it has an error.
KVSEP_HD uint64_t stop_candidate(uint64_t r, uint64_t err) { return err ? r : kNone; }
// *keep_before for the offsets pass: every run without a stop; the stop run and those before it (its good entries
// count), or only those before it when the error is the whole block's.
KVSEP_HD uint64_t keep_before(uint64_t stop, uint64_t err) {
  if (stop == kNone) return kNone;  // offsets::kKeepAll
  return err & kWhole ? stop : stop + 1;
}

// ---- the fill pass
// Lane r with base[r] = b, of either walk (emit as walk_run_as takes it).  b == kSkip: the run is past the stop, and
// nothing of the image is read.
template <bool kKeys, class R = Rule, class Rd, class Emit>
KVSEP_HD void fill_lane_as(Rd& rd, uint64_t ioff, uint64_t ilen, uint64_t r, uint64_t b, uint64_t limit, Emit&& emit) {
  if (b == kSkip || b >= limit) return;
  const Tail t = tail(rd, ioff, ilen);
  if (!t.ok || r >= t.nrestarts) return;
  const Run run = run_of(rd, ioff, t, r);
  if (!run.ok) return;
  walk_run_as<kKeys, R>(rd, ioff, run, t.restart_offset, emit);
}
// The plain walk: emit(k, off, len).
template <class R = Rule, class Rd, class Emit>
KVSEP_HD void fill_lane(Rd& rd, uint64_t ioff, uint64_t ilen, uint64_t r, uint64_t b, uint64_t limit, Emit&& emit) {
  fill_lane_as<false, R>(rd, ioff, ilen, r, b, limit,
                         [&](uint64_t k, uint64_t o, uint64_t l, uint64_t, uint64_t) { return emit(k, o, l); });
}
// ... and the keys walk: emit(k, off, len, key_at, key_len).
template <class R = Rule, class Rd, class Emit>
KVSEP_HD void fill_lane_keys(Rd& rd, uint64_t ioff, uint64_t ilen, uint64_t r, uint64_t b, uint64_t limit,
                             Emit&& emit) {
  fill_lane_as<true, R>(rd, ioff, ilen, r, b, limit, emit);
}

// How many elements hold handles of data blocks: the count cut to the room for them.
KVSEP_HD uint64_t held(uint64_t nblocks, uint64_t limit) { return nblocks < limit ? nblocks : limit; }
// The room for data blocks: the table form keeps two slots for the metaindex and index blocks (cap >= 2).
KVSEP_HD uint64_t data_cap(bool table, uint64_t cap) { return table ? cap - 2 : cap; }
// Element i >= m = held(...) of off / len: the table form's two footer handles (handles[0..4): all 0 after a bad
// footer), then padding.  which = 0 for off, 1 for len.
KVSEP_HD uint64_t after_data(bool table, uint64_t i, uint64_t m, const uint64_t* handles, int which) {
  return table && i - m < 2 ? handles[2 * (i - m) + which] : 0;
}
// The status a call ends with: the stop's code, else kCap when the table form's slots do not hold every block.
KVSEP_HD uint32_t final_status(uint32_t code, bool table, uint64_t nblocks, uint64_t cap) {
  if (code) return code;
  return table && nblocks > cap - 2 ? kCap : kOk;
}

// ---- the table form's read check
// How many of the cap slots hold a handle: none after a bad footer, else the data blocks and the footer's two.
KVSEP_HD uint64_t listed(uint32_t status, uint64_t nblocks, uint64_t cap) {
  return status == kBadFooter ? 0 : held(nblocks, cap - 2) + 2;
}
struct Prep {
  uint64_t len1;    // the bytes the checksum runs over: len + 1, or 0 (never dereferenced)
  bool read;        // the stored word is the image's, at off + len + 1
  uint32_t stored;  // ... else this
};
// Slot i of `real` listed ones: a usable handle is checked as ReadBlock checks it; a handle that leaves the image is
// reported bad without a byte of it being addressed; padding passes.
KVSEP_HD Prep prep(bool real, uint64_t off, uint64_t len, uint64_t n) {
  if (!real) return {0, false, kMaskOfZero};
  if (!usable(off, len, n)) return {0, false, kNoMatch};
  return {len + 1, true, 0};
}

}  // namespace sst
}  // namespace kvsep
