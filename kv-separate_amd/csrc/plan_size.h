// plan_size.h -- how a planned batch is cut into pieces and how large a plan a reservation must hold (no HIP:
// tests/cpp/plan_size_test.cc builds it alone).  crc32c_device.hip takes every number below from here: the piece size
// of a call (piece_for), the plan entries the call needs (pieces_needed) and the plan entries kvsep_crc32c_reserve
// allocates (pieces_reserved).  A captured call cannot allocate, so pieces_reserved(count, total) must be at least
// pieces_needed of every call of up to count blocks and total bytes, whichever piece size that call picks.
#pragma once
#include <algorithm>
#include <cstdint>

namespace kvsep {

constexpr uint64_t kSmallPiece = 16 * 1024;  // the automatic piece sizes are kSmallPiece << k, k = 0..2 (zsmall[k])
constexpr int kPlanWavesPerWg = 8;           // waves of the default CRC workgroup (kWgThreads / 64)

namespace plan {

// Pieces that give every wave of the persistent grid (one workgroup per CU) two of them.
inline uint64_t want_pieces(int num_cus) { return 2 * uint64_t(num_cus) * uint64_t(kPlanWavesPerWg); }

struct Piece {
  uint64_t bytes;
  int table;  // -1: the table of piece_bytes (zpiece); 0..2: zsmall[table]
};

// Piece size of a planned batch.  With the default setting (piece_auto), a batch too small to give every wave two
// pieces of piece_bytes gets 64, 32 or 16 KiB pieces instead: the largest size that still makes >= 2 pieces per wave,
// else 16 KiB (64 blocks of 1 MiB: 16 KiB pieces).  Batches with total_bytes / piece_bytes >= want_pieces keep
// piece_bytes, and so does every batch once the size was set explicitly.
inline Piece piece_for(uint64_t piece_bytes, bool piece_auto, int num_cus, uint64_t total_bytes) {
  Piece p{piece_bytes, -1};
  if (!piece_auto) return p;
  const uint64_t want = want_pieces(num_cus);
  for (int k = 2; k >= 0 && total_bytes / p.bytes < want; --k) p = Piece{kSmallPiece << k, k};
  return p;
}

// Plan entries of one call: a block of len bytes is cut into max(1, len / P) pieces (crc32c_plan_count_kernel), at
// most count + total_bytes / P in all, and one spare.
inline uint64_t pieces_needed(uint64_t piece, uint64_t count, uint64_t total_bytes) {
  return count + total_bytes / piece + 1;
}

// The most plan entries any call of up to count blocks and total_bytes bytes needs: for each piece size piece_for can
// return for a total <= total_bytes, the largest such total (pieces_needed grows with the total at a fixed size), and
// the maximum over the sizes.  Exact, not a bound: some call of that size needs every entry.
inline uint64_t pieces_budget(uint64_t piece_bytes, bool piece_auto, int num_cus, uint64_t count,
                              uint64_t total_bytes) {
  if (!piece_auto) return pieces_needed(piece_bytes, count, total_bytes);
  const uint64_t want = want_pieces(num_cus);
  // piece_for's choice is the first of these sizes whose threshold want * size the total reaches (16 KiB: always)
  const uint64_t sizes[4] = {piece_bytes, kSmallPiece << 2, kSmallPiece << 1, kSmallPiece};
  uint64_t hi = total_bytes;  // the largest total <= total_bytes that no earlier size takes
  uint64_t best = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t lo = i == 3 ? 0 : want * sizes[i];
    if (hi >= lo) best = std::max(best, pieces_needed(sizes[i], count, hi));
    if (lo == 0) break;
    hi = std::min(hi, lo - 1);
  }
  return best;
}

// Plan entries kvsep_crc32c_reserve(count, total_bytes) provides: the budget of the caller's own numbers plus the one
// byte per block that the SST read check adds (it runs len + 1 per block: a batch of total_bytes + count bytes).
inline uint64_t pieces_reserved(uint64_t piece_bytes, bool piece_auto, int num_cus, uint64_t count,
                                uint64_t total_bytes) {
  const uint64_t with_type_bytes = total_bytes + count < total_bytes ? ~uint64_t(0) : total_bytes + count;
  return pieces_budget(piece_bytes, piece_auto, num_cus, count, with_type_bytes);
}

}  // namespace plan
}  // namespace kvsep
