// vlog_run.h -- the rules of the device value-log reader (no HIP, no allocation: tests/cpp/vlog_run_test.cc builds it
// alone, with a tiny window, and runs the kernels' control flow lane by lane against a plain serial walk).  The kernels
// (crc32c_vlogwalk.inc) take every index and byte decision from here: whether a header and its payload lie in the image
// (has_header, has_payload), what a header says (header_stored, header_len), where the next one is (next_header), which
// bytes a refill stages and in which 16-byte granules (skew, window_hi, granule_count, granule_addr), whether a header
// is read from the window or refills it (staged, lds_index), how records leave the wave (emit_lane, batch_full,
// emit_index, emit_store), what the arrays hold past the records (held, pad_first, kPadStored) and what the read form
// reports (good_count, good_bytes, drop_bytes).
//
// The reader is VlogReader::ReadRecord (db/value_log_reader.cc:86-138), as kvsep_vlog_walk (framing.cpp) restates it on
// the host: records [Mask(crc) LE32][len LE32][payload] back to back from offset 0; a header or a payload that runs
// past the end of the image is eof.  The chain of headers is serial in one 64-bit number, the position p of the next
// header; one wavefront follows it.  A naive loop pays one HBM round trip per record.  This one stages a window of the
// image in LDS with one batch of independent 16-byte loads and steps inside it at LDS latency: a refill only when the
// next header is not wholly staged.
//
// Termination: every step passes has_header and has_payload and then advances p by kHeader + l >= 8 with
// p + kHeader + l <= n, so the loop runs at most n / 8 times (max_steps); a refill happens inside a step, at most once
// (a header at p is always staged by a refill at p: has_header holds and kWindow >= kGranule + kHeader).  Nothing
// else in the walk loops on data; the padding loop runs cap / 64 times at most.
// Widths: p, n, k and cap are 64-bit; a position inside the window (p - lo + skew) is below kWindow and fits 32 bits.
#pragma once
#include <cstdint>

#include "concat_run.h"  // KVSEP_HD

#ifndef KVSEP_VLOG_WINDOW
// Shipped window: the lowest summed walk time over 1 MiB, 100-byte and empty records of 4, 16 and 32 KiB -- by less
// than the spread between runs; the step, not the refill, is what the walk costs (profiles/round14/vlog_read_cost.txt,
// DESIGN.md §4).
#define KVSEP_VLOG_WINDOW 32768
#endif

namespace kvsep {
namespace vlogrun {

constexpr uint64_t kHeader = 8;    // db/log_format.h:40: the stored checksum word, then the length word
constexpr uint64_t kGranule = 16;  // a load is one naturally aligned 16-byte granule
constexpr uint32_t kLanes = 64;    // the walk is one workgroup of one wavefront
constexpr uint64_t kWindow = KVSEP_VLOG_WINDOW;  // bytes staged per refill
constexpr uint32_t kGranules = uint32_t(kWindow / kGranule);
constexpr uint32_t kLoadsPerLane = (kGranules + kLanes - 1) / kLanes;  // all issued before the first wait
constexpr uint32_t kLdsSlack = 8;  // the header read takes three aligned words: up to 3 + 4 bytes past the header
constexpr uint32_t kPadStored = 0xa282ead8u;  // kvsep_crc32c_mask(0): an empty block with this word passes the verify
static_assert(kWindow % kGranule == 0 && kWindow >= 2 * kGranule && kWindow <= 65536 - kGranule,
              "the window is whole granules, holds a header at any skew and fits the LDS");

// ---- the image
// p <= n always (the walk starts at 0 and only moves to next_header of a record that has_payload).
KVSEP_HD bool has_header(uint64_t p, uint64_t n) { return n - p >= kHeader; }  // p + 8 <= n without the sum
// The payload test of a header at p (has_header): l <= n - p - 8.  No sum of p and l: a length word of 0xFFFFFFFF in
// a 20-byte image is eof, not a wrapped small number.
KVSEP_HD bool has_payload(uint64_t p, uint64_t l, uint64_t n) { return l <= n - p - kHeader; }
KVSEP_HD uint32_t header_stored(uint64_t h) { return uint32_t(h); }  // h = the header's 8 bytes, little-endian
KVSEP_HD uint64_t header_len(uint64_t h) { return h >> 32; }
KVSEP_HD uint64_t rec_off(uint64_t p) { return p + kHeader; }
KVSEP_HD uint64_t next_header(uint64_t p, uint64_t l) { return p + kHeader + l; }  // <= n by has_payload
KVSEP_HD uint64_t max_steps(uint64_t n) { return n / kHeader; }

// ---- the window
// A refill at header position p (has_header) stages the granules from the one that holds byte p: the image bytes
// [p, window_hi) are then in LDS, byte q at lds_index(q, p, skew).  `addr` = the address of image byte 0, any alignment.
KVSEP_HD uint32_t skew(uint64_t addr, uint64_t p) { return uint32_t((addr + p) & (kGranule - 1)); }
// One past the last staged image byte: the window's kWindow bytes start `skew` bytes before p and stop at the image's end.
KVSEP_HD uint64_t window_hi(uint64_t p, uint32_t sk, uint64_t n) {
  return n - p > kWindow - sk ? p + (kWindow - sk) : n;
}
// The granules of [p, hi): 1 .. kGranules, every one holds at least one byte of [p, hi) and so of the image.
KVSEP_HD uint32_t granule_count(uint64_t p, uint32_t sk, uint64_t hi) {
  return uint32_t((sk + (hi - p) + kGranule - 1) / kGranule);
}
KVSEP_HD uint64_t granule_addr(uint64_t addr, uint64_t p, uint32_t sk, uint32_t j) {
  return addr + p - sk + uint64_t(j) * kGranule;
}
// Lane `lane`'s r-th load of a refill: granule lane + r * kLanes, clamped to the last granule so that the batch has no
// branch (a repeated load of a granule of the image; its LDS slot lies past window_hi and is never read).
KVSEP_HD uint32_t load_slot(uint32_t lane, uint32_t r) { return lane + r * kLanes; }
KVSEP_HD bool slot_in_lds(uint32_t slot) { return slot < kGranules; }
KVSEP_HD uint32_t load_granule(uint32_t slot, uint32_t count) { return slot < count ? slot : count - 1; }
// The refill rule: the header at q is read from the window [lo, hi) only if all 8 of its bytes are staged.
KVSEP_HD bool staged(uint64_t q, uint64_t lo, uint64_t hi) { return q >= lo && q <= hi && hi - q >= kHeader; }
KVSEP_HD uint32_t lds_index(uint64_t q, uint64_t lo, uint32_t sk) { return uint32_t(q - lo) + sk; }
// The header's bytes from the three aligned LDS words that hold them: w0 at lds_word(idx), then the next two.
KVSEP_HD uint32_t lds_word(uint32_t idx) { return idx >> 2; }
KVSEP_HD uint64_t header_of_words(uint32_t idx, uint32_t w0, uint32_t w1, uint32_t w2) {
  const uint32_t s = 8 * (idx & 3);
  const uint64_t lo = uint64_t(w0) | (uint64_t(w1) << 32);
  return s ? (lo >> s) | (uint64_t(w2) << (64 - s)) : lo;
}

// ---- the emission batch
// Record k is held by lane k % 64 until 64 are collected (or the walk ends); the batch [first, first + cnt) is then
// stored coalesced, lane i storing element first + i, masked by the arrays' capacity.
KVSEP_HD uint32_t emit_lane(uint64_t k) { return uint32_t(k & (kLanes - 1)); }
KVSEP_HD bool batch_full(uint64_t k) { return (k & (kLanes - 1)) == 0; }  // after ++k
KVSEP_HD uint64_t batch_first(uint64_t k, uint32_t cnt) { return k - cnt; }
KVSEP_HD uint32_t tail_count(uint64_t k) { return uint32_t(k & (kLanes - 1)); }
KVSEP_HD uint64_t emit_index(uint64_t first, uint32_t lane) { return first + lane; }
KVSEP_HD bool emit_store(uint32_t lane, uint32_t cnt, uint64_t i, uint64_t cap) { return lane < cnt && i < cap; }

// ---- the padding: off = len = 0 and stored = kPadStored from held to cap, lane `lane` taking held + lane, + 64, ...
KVSEP_HD uint64_t held(uint64_t nrec, uint64_t cap) { return nrec < cap ? nrec : cap; }
KVSEP_HD uint64_t pad_first(uint64_t nrec, uint64_t cap, uint32_t lane) { return held(nrec, cap) + lane; }

// ---- the totals of the read form (kvsep_vlog_verify_host's, value_log_reader.cc:109-122)
// first_bad = the verify call's lowest failing index over all cap elements, ~0 for none; the padding passes, so it is a
// record's index or none.  g = the leading records among the first held(nrec, cap) that pass.
KVSEP_HD uint64_t good_count(uint64_t first_bad, uint64_t nrec, uint64_t cap) {
  const uint64_t c = held(nrec, cap);
  return first_bad < c ? first_bad : c;
}
KVSEP_HD bool has_good(uint64_t g) { return g != 0; }                      // good_bytes = off[g - 1] + len[g - 1]
KVSEP_HD bool has_drop(uint64_t g, uint64_t nrec, uint64_t cap) { return g < held(nrec, cap); }  // drop_bytes = len[g]

}  // namespace vlogrun
}  // namespace kvsep
