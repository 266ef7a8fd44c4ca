// crc32c_pack.inc -- crc32c_pack_kernel, the batched byte-exact gather-copy with frame stamping (included once, inside
// namespace kvsep, by crc32c_device.hip).  Block i of a batch is the run of segments [first[i], first[i + 1]); their
// bytes go back to back to dst + dst_off[i] + lead, and the frame type adds the bytes the reference's writers put around
// them:
//   PackPlain  nothing                                                        (kvsep_crc32c_pack_device)
//   PackVlog   [Mask(crc[i]) LE32][len_i LE32] in front, lead = 8             (db/value_log_writer.cc:46-76)
//   PackSst    [types[i]][crc[i] LE32] behind, crc[i] the masked trailer word (table/table_builder.cc:209-232)
//   PackLog    [Mask(crc[i]) LE32][len_i LE16][types[i]] in front, lead = 7      (db/log_writer.cc:84-115)
// A framed block that does not lie inside [0, dst_bytes) is not written at all.
//
// Every index and byte decision comes from pack_run.h, which tests/cpp/pack_run_test.cc runs lane by lane on the CPU.
// Stores are byte-exact: the bytes before the first and after the last 16-B boundary of a destination range are byte
// stores, the granules between are naturally aligned 16-B stores whose bytes come from one source granule, or from two
// consecutive ones joined by v_alignbyte_b32.  Nothing is read-modify-written, so blocks that share a granule, written
// by different waves, never see each other.  Loads stay inside the naturally aligned 16-B granules that hold a byte of
// a segment; a segment of length 0 is never dereferenced.  first is read for count + 1 elements and clamped to nseg,
// dst_off / crc / types for count.  No scratch, no atomics, no LDS, one launch.
//
// Work split.  One wavefront copies one tile (pack::kTile payload bytes) of one block at a time; it walks the run in
// passes of 64 segments (lane l holds segment l's descriptor, the loop over them reads lanes: wave-uniform, full EXEC)
// and copies each part of a segment inside the tile as a span of its own.  The grid has two parts:
//   workgroups [0, short_wgs)  a wave reads the descriptors of pack::kShortBlocks consecutive blocks lane-parallel and
//                              copies those of one tile, one after another;
//   the rest                   pack::kChunkBlocks consecutive blocks are a chunk, `team` workgroups share a chunk: every
//                              wave of the team reads the chunk's descriptors and takes the tiles of its longer blocks
//                              that pack::first_tile deals to it.  A batch of one 1 GiB record runs on every CU.
// The host cannot know which part a block belongs to (the lengths are on the device), so both parts always run; the
// second costs a descriptor read where no block is long.

// kPackThreads, kPackWaves and the grid (pack::short_wgs, pack::chunk_count, pack::team_size): pack_run.h

struct PackPlain {
  static constexpr pack::Frame kFrame = pack::kPlain;
};
struct PackVlog {
  static constexpr pack::Frame kFrame = pack::kVlog;
};
struct PackSst {
  static constexpr pack::Frame kFrame = pack::kSst;
};
struct PackLog {
  static constexpr pack::Frame kFrame = pack::kLog;
};

struct PackArgs {
  const uint8_t* base;
  const uint64_t* seg_off;
  const uint64_t* seg_len;
  const uint64_t* first;  // null: block i is segment i (the SST form)
  uint8_t* dst;
  uint64_t dst_bytes;
  const uint64_t* dst_off;
  uint64_t count, nseg;
  const uint32_t* crc;   // PackVlog / PackLog: the CRC, masked here; PackSst: the trailer word as it is stored
  const uint8_t* types;  // PackSst, PackLog
  uint32_t short_wgs;    // workgroups of the first part of the grid
  uint32_t team;         // workgroups per chunk in the second
};

// Global (not flat) address space, as the CRC kernels' loads.  Plain loads and stores: non-temporal ones are not
// measured for this kernel (DESIGN.md §4).
typedef __attribute__((address_space(1))) uint8_t gu8;
typedef __attribute__((address_space(1))) u32x4 gwu32x4;
__device__ __forceinline__ uint8_t pack_ld8(uintptr_t a) { return *reinterpret_cast<const gu8*>(a); }
__device__ __forceinline__ void pack_st8(uintptr_t a, uint8_t v) { *reinterpret_cast<gu8*>(a) = v; }
__device__ __forceinline__ void pack_st16(uintptr_t a, const uint32_t w[4]) {
  u32x4 v;
  v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
  *reinterpret_cast<gwu32x4*>(a) = v;
}

template <bool kShift>
__device__ __forceinline__ void pack_body(const pack::Span& s, uint32_t lane) {
  const uint64_t iters = pack::body_iters(s);
  for (uint64_t it = 0; it < iters; ++it) {
    uint64_t g[pack::kUnroll];
    uint4 lo[pack::kUnroll], hi[pack::kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < pack::kUnroll; ++u) {
      g[u] = pack::body_granule(s, it, u, lane);
      lo[u] = hi[u] = make_uint4(0, 0, 0, 0);
      if (g[u]) {
        const uint64_t a = pack::body_src(s, g[u]);
        lo[u] = ld16(a);
        if constexpr (kShift) hi[u] = ld16(a + pack::kGran);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < pack::kUnroll; ++u) {
      if (!g[u]) continue;
      const uint32_t l[4] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w};
      if constexpr (kShift) {
        const uint32_t h[4] = {hi[u].x, hi[u].y, hi[u].z, hi[u].w};
        uint32_t out[4];
        pack::align16(l, h, s.sh, out);
        pack_st16(g[u], out);
      } else {
        pack_st16(g[u], l);
      }
    }
  }
}

// One span: n >= 1 bytes from src to dst (wave-uniform).  Lanes 0..31 copy the edge bytes, then every lane body granules.
__device__ __forceinline__ void pack_span(uintptr_t src, uintptr_t dst, uint64_t n, uint32_t lane) {
  const pack::Span s = pack::split(src, dst, n);
  const uint64_t e = pack::edge_byte(s, lane);
  if (e != ~uint64_t(0)) pack_st8(dst + e, pack_ld8(src + e));
  if (s.body0 == s.body1) return;
  if (s.sh == 0) pack_body<false>(s, lane);
  else pack_body<true>(s, lane);
}

// Tile t of the block whose run is r, payload `total` bytes, payload at dst + at.
__device__ __forceinline__ void pack_tile(const PackArgs& a, pack::Run r, uint64_t total, uint64_t at, uint64_t t,
                                          uint32_t lane) {
  const pack::Range tr = pack::tile_range(total, t);
  uint64_t pos = 0;
  for (uint64_t ps = r.s; ps < r.e && pos < tr.b;) {
    const uint32_t n = pack::pass_segs(ps, r.e);
    uint64_t so = 0, sl = 0;
    if (lane < n) {
      sl = a.seg_len[ps + lane];
      so = a.seg_off[ps + lane];
    }
    for (uint32_t k = 0; k < n && pos < tr.b; ++k) {
      const uint64_t len = concat_readlane64(sl, int(k)), off = concat_readlane64(so, int(k));
      const pack::Cut c = pack::cut_segment(pos, len, tr);
      if (c.n)
        pack_span(reinterpret_cast<uintptr_t>(a.base) + off + c.skip, reinterpret_cast<uintptr_t>(a.dst) + at + c.pos,
                  c.n, lane);
      pos += len;
    }
    ps += n;
  }
}

template <typename F>
__global__ void __launch_bounds__(kPackThreads) crc32c_pack_kernel(PackArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool long_part = blockIdx.x >= a.short_wgs;
  uint64_t b0;
  uint32_t nb, my = 0, team_waves = 1;
  if (!long_part) {
    b0 = (uint64_t(blockIdx.x) * kPackWaves + wv) * pack::kShortBlocks;
    nb = pack::kShortBlocks;
  } else {
    const uint32_t w = blockIdx.x - a.short_wgs;
    b0 = uint64_t(w / a.team) * pack::kChunkBlocks;
    nb = pack::kChunkBlocks;
    my = (w % a.team) * kPackWaves + wv;
    team_waves = a.team * kPackWaves;
  }
  const uint64_t b = b0 + lane;
  pack::Run r{0, 0};
  uint64_t total = 0, d = 0;
  bool take = false;
  if (lane < nb && b < a.count) {
    r = a.first ? pack::clamp_run(a.first[b], a.first[b + 1], a.nseg) : pack::clamp_run(b, b + 1, a.nseg);
    for (uint64_t j = r.s; j < r.e; ++j) total = pack::add_sat(total, a.seg_len[j]);
    d = a.dst_off[b];
    take = pack::fits(d, total, F::kFrame, a.dst_bytes) && (pack::tile_count(total) > 1) == long_part;
  }
  // the blocks of this part, one at a time on all 64 lanes (wave-uniform from here on)
  for (uint64_t todo = __builtin_amdgcn_ballot_w64(take); todo; todo &= todo - 1) {
    const int src = __builtin_ctzll(todo);
    const pack::Run run{concat_readlane64(r.s, src), concat_readlane64(r.e, src)};
    const uint64_t tot = concat_readlane64(total, src), at = concat_readlane64(d, src);
    const uint64_t tiles = pack::tile_count(tot);
    for (uint64_t t = pack::first_tile(uint32_t(src), my, team_waves); t < tiles; t += team_waves) {
      if (t == 0) {  // the frame bytes go with the first tile
        const uintptr_t rec = reinterpret_cast<uintptr_t>(a.dst) + at;
        if constexpr (F::kFrame == pack::kVlog) {
          const uint32_t masked = mask_crc(a.crc[b0 + uint32_t(src)]);
          if (lane < 8) pack_st8(rec + lane, pack::vlog_header_byte(masked, tot, lane));
        }
        if constexpr (F::kFrame == pack::kSst) {
          const uint32_t word = a.crc[b0 + uint32_t(src)];
          const uint8_t type = a.types[b0 + uint32_t(src)];
          if (lane < 5) pack_st8(rec + tot + lane, pack::sst_trailer_byte(type, word, lane));
        }
        if constexpr (F::kFrame == pack::kLog) {
          const uint32_t masked = mask_crc(a.crc[b0 + uint32_t(src)]);
          const uint8_t type = a.types[b0 + uint32_t(src)];
          if (lane < 7) pack_st8(rec + lane, pack::log_header_byte(masked, tot, type, lane));
        }
      }
      pack_tile(a, run, tot, at + pack::lead(F::kFrame), t, lane);
    }
  }
}
