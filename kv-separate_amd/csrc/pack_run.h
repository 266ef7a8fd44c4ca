// pack_run.h -- the geometry of crc32c_pack_kernel (no HIP, no allocation: tests/cpp/pack_run_test.cc builds it alone and
// runs it lane by lane against memcpy).  The kernel (crc32c_pack.inc) takes every index and byte decision below from
// here: which segments a block's run holds (concat::clamp_run, shared with the combine), whether a framed block lies
// inside the destination (fits), how a block's payload is cut into tiles (tile_count, tile_range, tile_owner), which
// part of a segment falls into a tile (cut_segment), how a destination range is cut into byte-granular edges and
// naturally aligned 16-B body stores (split, edge_byte, body_granule), which source granules a body store reads
// (body_src) and how two of them give the 16 bytes stored (align16).
//
// A block is the bytes of its run's segments back to back, `lead` frame bytes before them and `trail` after.  One
// wavefront copies one tile of a block: it walks the run, and every non-empty intersection of a segment with the tile is
// a span (src, dst, n) copied on its own -- byte stores for the bytes before the first and after the last 16-B boundary
// of [dst, dst + n), 16-B stores for the granules between.  No store is wider than the bytes it owns, so two spans that
// meet inside a granule (two segments, two tiles, two blocks, written by different waves) never touch each other's bytes.
#pragma once
#include <cstdint>

#include "concat_run.h"

namespace kvsep {

// crc32c_pack_kernel's workgroup (crc32c_pack.inc); here so that host-only code can include it.
constexpr uint32_t kPackThreads = 256;
constexpr uint32_t kPackWaves = kPackThreads / 64;

namespace pack {

using concat::Run;
using concat::clamp_run;

constexpr uint64_t kGran = 16;  // the load / store granule
// Payload bytes one wavefront copies as one unit of work.  64 KiB is 16 iterations of the body loop below: long enough
// that the walk to the tile's first segment and the two edge stores are noise, short enough that a 1 MiB record gives
// 16 waves work and a 1 GiB one every CU.
constexpr uint64_t kTile = 64 * 1024;
constexpr uint32_t kWaveLanes = 64;
// Body granules per lane and loop iteration: 4 (8 loads in flight per lane when source and destination are shifted
// against each other), 4 KiB per wavefront and iteration.
constexpr uint32_t kUnroll = 4;
constexpr uint64_t kIterBytes = uint64_t(kWaveLanes) * kGran * kUnroll;
// Blocks whose descriptors one wavefront reads lane-parallel: 8 in the part of the grid that copies one-tile blocks (a
// wavefront then copies its blocks one after another, so fewer blocks per wave than the combine's 16 keep more waves,
// and so more bytes, in flight), 64 -- one chunk -- in the part that shares out the tiles of longer blocks.
constexpr uint32_t kShortBlocks = 8;
constexpr uint32_t kChunkBlocks = 64;
// Workgroups that share the long blocks of one chunk, at least: a batch of very many blocks still gives a long block
// kMinTeam workgroups.
constexpr uint32_t kMinTeam = 4;

// Frame bytes before and after the payload: vlog records carry [Mask(crc) LE32][len LE32] in front, SST blocks
// [type][Mask(crc) LE32] behind, log / MANIFEST fragments [Mask(crc) LE32][len LE16][type] in front.
enum Frame : uint32_t { kPlain = 0, kVlog = 1, kSst = 2, kLog = 3 };
KVSEP_HD uint64_t lead(Frame f) { return f == kVlog ? 8 : f == kLog ? 7 : 0; }
KVSEP_HD uint64_t trail(Frame f) { return f == kSst ? 5 : 0; }

// Sums of lengths saturate at 2^64 - 1, the value fits() refuses: a run whose bytes leave 64 bits fits nowhere.
constexpr uint64_t kSaturated = ~uint64_t(0);
KVSEP_HD uint64_t add_sat(uint64_t a, uint64_t b) { return a + b < a ? kSaturated : a + b; }

// Whether [dst_off, dst_off + lead + payload + trail) lies inside [0, dst_bytes).  No sum is formed that can wrap; a
// payload of kSaturated is a sum that did (no buffer holds 2^64 - 1 bytes, so no real block is refused by this).
// dst_off = 2^64 - 1 is the offsets pass's mark for a block that is not laid out (offsets::kSkip): it is refused for
// every payload and frame, but for an empty plain block in a destination of 2^64 - 1 bytes, which fits and writes
// nothing (tests/cpp/offsets_run_test.cc).
KVSEP_HD bool fits(uint64_t dst_off, uint64_t payload, Frame f, uint64_t dst_bytes) {
  if (dst_off > dst_bytes || payload == kSaturated) return false;
  const uint64_t room = dst_bytes - dst_off, frame = lead(f) + trail(f);
  return frame <= room && payload <= room - frame;
}

// Tiles of a payload of `total` bytes: one for everything up to kTile (an empty payload too: its frame bytes are
// written with tile 0), else ceil(total / kTile).
KVSEP_HD uint64_t tile_count(uint64_t total) { return total <= kTile ? 1 : (total - 1) / kTile + 1; }

// Payload positions [t0, t1) of tile t < tile_count(total).
struct Range {
  uint64_t a, b;
};
KVSEP_HD Range tile_range(uint64_t total, uint64_t t) {
  const uint64_t a = t * kTile;
  return {a, total - a < kTile ? total : a + kTile};
}

// The long part of the grid: chunk c holds blocks [c * kChunkBlocks, + kChunkBlocks), `team` workgroups share its
// long blocks.  The team shrinks as the batch grows (about `wgs` workgroups in all) down to kMinTeam.
KVSEP_HD uint64_t chunk_count(uint64_t count) { return (count + kChunkBlocks - 1) / kChunkBlocks; }
KVSEP_HD uint32_t team_size(uint64_t count, uint32_t wgs) {
  const uint64_t t = wgs / chunk_count(count ? count : 1);
  return uint32_t(t < kMinTeam ? kMinTeam : t);
}
// The first part of the grid: short_wgs workgroups whose waves take kShortBlocks blocks each (then `team` workgroups per
// chunk: short_wgs + chunk_count * team in all).
KVSEP_HD uint32_t short_wgs(uint64_t count) {
  constexpr uint64_t per_wg = uint64_t(kPackWaves) * kShortBlocks;
  return uint32_t((count + per_wg - 1) / per_wg);
}
// Tile t of the block in lane `slot` of its chunk goes to wave (slot + t) mod team_waves of the chunk's team: the tiles
// of one block go round the team, and the first tiles of neighbouring blocks start on different waves.
KVSEP_HD bool tile_owner(uint32_t slot, uint64_t t, uint32_t wave, uint32_t team_waves) {
  return (t + slot) % team_waves == wave;
}
// The same as a walk: wave `wave` takes tile first_tile and every team_waves-th after it (the kernel's loop: one 32-bit
// remainder a block, where asking tile_owner for every tile would be a 64-bit one a tile).
KVSEP_HD uint64_t first_tile(uint32_t slot, uint32_t wave, uint32_t team_waves) {
  return (wave + team_waves - slot % team_waves) % team_waves;
}

// The part of a segment at payload positions [pos, pos + len) that tile [t.a, t.b) holds: `skip` bytes into the
// segment, at payload position `pos`, `n` bytes (0: none).
struct Cut {
  uint64_t skip, pos, n;
};
KVSEP_HD Cut cut_segment(uint64_t pos, uint64_t len, Range t) {
  const uint64_t a = pos > t.a ? pos : t.a;
  const uint64_t end = pos + len;  // <= total: no wrap once the block fits
  const uint64_t b = end < t.b ? end : t.b;
  return b > a ? Cut{a - pos, a, b - a} : Cut{0, a, 0};
}

// A span of n >= 1 bytes from address src to address dst: head [dst, body0) and tail [body1, dst + n) are byte-granular
// and shorter than 16 bytes each, [body0, body1) is whole aligned granules (body0 == body1: none; then the head takes the
// bytes up to the boundary inside the span, if there is one, and the tail the rest).  sh = the byte shift between a
// destination granule and the source granule that holds its first byte.
struct Span {
  uint64_t src, dst, n;
  uint64_t body0, body1;
  uint32_t sh;
};
KVSEP_HD Span split(uint64_t src, uint64_t dst, uint64_t n) {
  const uint64_t end = dst + n;
  uint64_t b0 = (dst + kGran - 1) & ~(kGran - 1);
  uint64_t b1 = end & ~(kGran - 1);
  if (b0 > end) b0 = end;  // the span lies inside one granule: all head
  if (b1 < b0) b1 = b0;
  return {src, dst, n, b0, b1, uint32_t((src - dst) & (kGran - 1))};
}

// Lanes 0..15 hold the head's bytes, lanes 16..31 the tail's: the offset into the span of the byte `lane` copies, or
// ~0 for a lane with none.
KVSEP_HD uint64_t edge_byte(const Span& s, uint32_t lane) {
  if (lane < kGran) return lane < s.body0 - s.dst ? lane : ~uint64_t(0);
  const uint64_t i = lane - kGran;
  return lane < 2 * kGran && i < s.dst + s.n - s.body1 ? s.body1 - s.dst + i : ~uint64_t(0);
}

// Iterations of the body loop, and the destination granule (an address) of lane `lane` in unroll slot u of iteration
// it, or 0 past the body.
KVSEP_HD uint64_t body_iters(const Span& s) { return (s.body1 - s.body0 + kIterBytes - 1) / kIterBytes; }
KVSEP_HD uint64_t body_granule(const Span& s, uint64_t it, uint32_t u, uint32_t lane) {
  const uint64_t g = s.body0 + ((it * kUnroll + u) * kWaveLanes + lane) * kGran;
  return g < s.body1 ? g : 0;
}
// The aligned source granule holding the first byte stored to destination granule g; with sh != 0 the store also needs
// the granule after it (which holds the 16th byte: a byte of the span, since g + 16 <= dst + n).
KVSEP_HD uint64_t body_src(const Span& s, uint64_t g) { return (s.src + (g - s.dst)) & ~(kGran - 1); }

// Bytes sh .. sh + 15 of the 32 bytes lo || hi (little-endian words), 1 <= sh <= 15.
KVSEP_HD uint32_t align_word(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
  return uint32_t(((uint64_t(hi) << 32) | lo) >> (8 * r));
#endif
}
KVSEP_HD void align16(const uint32_t lo[4], const uint32_t hi[4], uint32_t sh, uint32_t out[4]) {
  const uint32_t r = sh & 3u;
  switch (sh >> 2) {  // constant indices in every arm: the words stay in registers
    case 0:
      out[0] = align_word(lo[1], lo[0], r), out[1] = align_word(lo[2], lo[1], r);
      out[2] = align_word(lo[3], lo[2], r), out[3] = align_word(hi[0], lo[3], r);
      break;
    case 1:
      out[0] = align_word(lo[2], lo[1], r), out[1] = align_word(lo[3], lo[2], r);
      out[2] = align_word(hi[0], lo[3], r), out[3] = align_word(hi[1], hi[0], r);
      break;
    case 2:
      out[0] = align_word(lo[3], lo[2], r), out[1] = align_word(hi[0], lo[3], r);
      out[2] = align_word(hi[1], hi[0], r), out[3] = align_word(hi[2], hi[1], r);
      break;
    default:
      out[0] = align_word(hi[0], lo[3], r), out[1] = align_word(hi[1], hi[0], r);
      out[2] = align_word(hi[2], hi[1], r), out[3] = align_word(hi[3], hi[2], r);
      break;
  }
}

// A run is walked in passes of up to 64 segments: lane l of a pass holds segment ps + l.
KVSEP_HD uint32_t pass_segs(uint64_t ps, uint64_t e) { return e - ps < kWaveLanes ? uint32_t(e - ps) : kWaveLanes; }

// The frame bytes, as the writers lay them down: byte i of the vlog header [Mask(crc) LE32][len LE32] (the length's low
// 32 bits), of the SST trailer [type][Mask(crc) LE32] and of the log fragment header.
KVSEP_HD uint8_t vlog_header_byte(uint32_t masked, uint64_t len, uint32_t i) {
  return uint8_t((i < 4 ? masked : uint32_t(len)) >> (8 * (i & 3u)));
}
KVSEP_HD uint8_t sst_trailer_byte(uint8_t type, uint32_t masked, uint32_t i) {
  return i == 0 ? type : uint8_t(masked >> (8 * (i - 1)));
}
// Byte i of the log fragment header [Mask(crc) LE32][len LE16][type] (db/log_writer.cc:84-115; a fragment's length is
// at most 32,761).
KVSEP_HD uint8_t log_header_byte(uint32_t masked, uint64_t len, uint8_t type, uint32_t i) {
  return i < 4 ? uint8_t(masked >> (8 * i)) : i < 6 ? uint8_t(len >> (8 * (i - 4))) : type;
}

}  // namespace pack
}  // namespace kvsep
