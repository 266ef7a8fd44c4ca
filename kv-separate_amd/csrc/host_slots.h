// host_slots.h -- how a host-memory call is cut into staging-slot jobs (no HIP, no allocation:
// tests/cpp/host_slots_test.cc builds it alone).  crc32c_host.cpp takes every grouping decision below from here: which
// block is too long for a slot and runs as a chain of segments (is_long, segment_count, segment), which consecutive
// blocks of the span form share one staged range (span_group, span_at) and which blocks of the pointer-per-block form
// are packed into one slot and where (gather_group).  Two limits bound a job: the bytes of a slot (kSlotBytes) and the
// descriptor entries of a slot (kSlotBlocks).
#pragma once
#include <algorithm>
#include <cstdint>

namespace kvsep {

constexpr uint64_t kSlotBytes = 64ull << 20;  // one pinned / device staging slot
constexpr uint64_t kSlotBlocks = 1ull << 16;  // blocks (descriptor, init and result entries) of one slot job

namespace slots {

// A block over the slot size runs alone, as a chain of segments; a block of exactly slot_bytes still fits a group.
inline bool is_long(uint64_t len, uint64_t slot_bytes) { return len > slot_bytes; }

// The segment chain of a long block of n bytes: every segment is slot_bytes long and the last takes the remainder.
// Segment k is seeded with the CRC of segment k - 1 (the caller's init for k = 0).
inline uint64_t segment_count(uint64_t n, uint64_t slot_bytes) { return n / slot_bytes + (n % slot_bytes ? 1 : 0); }

struct Segment {
  uint64_t at, bytes;  // [at, at + bytes) of the block
};
inline Segment segment(uint64_t n, uint64_t k, uint64_t slot_bytes) {
  const uint64_t at = k * slot_bytes;
  return {at, std::min(slot_bytes, n - at)};
}

// The span form: blocks [i, j) are staged as the one range [lo, hi) of the caller's span that covers them, block k at
// span_at(off[k], group) of the slot.  The group takes consecutive blocks, whatever order their offsets come in, while
// the covering range (empty blocks' offsets included) stays within slot_bytes, up to max_blocks of them, and stops
// before a long block.  Block i itself must not be long.  max_len: the longest block of the group.
struct SpanGroup {
  uint64_t j, lo, hi, max_len;
};
inline SpanGroup span_group(const uint64_t* off, const uint64_t* len, uint64_t i, uint64_t count, uint64_t slot_bytes,
                            uint64_t max_blocks) {
  SpanGroup g{i + 1, off[i], off[i] + len[i], len[i]};
  while (g.j < count && g.j - i < max_blocks && !is_long(len[g.j], slot_bytes)) {
    const uint64_t nlo = std::min(g.lo, off[g.j]), nhi = std::max(g.hi, off[g.j] + len[g.j]);
    if (nhi - nlo > slot_bytes) break;
    g.lo = nlo;
    g.hi = nhi;
    g.max_len = std::max(g.max_len, len[g.j]);
    ++g.j;
  }
  return g;
}
// Where a block of the group starts in the staged range: relative to the group's final lo, never to a block's own off.
inline uint64_t span_at(uint64_t off, const SpanGroup& g) { return off - g.lo; }

// The pointer-per-block form: blocks [i, j) are packed into one slot back to back, block k at at[k - i], each start
// rounded up to 16 B; used = the end of the last block (the bytes to move to the device).  A block joins while it
// still ends within slot_bytes after the round-up, up to max_blocks of them, and the group stops before a long block.
// Block i itself must not be long.  An empty block gets the offset a block would get there and has nothing to copy.
// at must have room for min(count - i, max_blocks) entries.
struct GatherGroup {
  uint64_t j, used, max_len;
};
inline GatherGroup gather_group(const uint64_t* len, uint64_t i, uint64_t count, uint64_t slot_bytes,
                                uint64_t max_blocks, uint64_t* at) {
  GatherGroup g{i, 0, 0};
  while (g.j < count && g.j - i < max_blocks && !is_long(len[g.j], slot_bytes)) {
    const uint64_t a = (g.used + 15) & ~uint64_t(15);
    if (a + len[g.j] > slot_bytes) break;
    at[g.j - i] = a;
    g.max_len = std::max(g.max_len, len[g.j]);
    g.used = a + len[g.j];
    ++g.j;
  }
  return g;
}

}  // namespace slots
}  // namespace kvsep
