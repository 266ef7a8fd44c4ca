// crc32c_concat.inc -- crc32c_concat_kernel, the batched CRC combine (included once, inside namespace kvsep, by
// crc32c_device.hip).  Block i of a batch is the run of segments [first[i], first[i + 1]) and
//   out[i] = fold over the run of  acc <- acc * X(seg_len[j]) ^ seg_crc[j],  acc starting at init[i] (0 without init),
// which is Extend(init[i], the segments' bytes back to back) when seg_crc[j] = Value(segment j) (gf2.h combine).  Only
// CRC values and lengths are read, never payload, so a length may be anything up to 2^64 - 1.
//
// Every index decision comes from concat_run.h, which tests/cpp/concat_run_test.cc runs on the CPU: first[] values are
// clamped to nseg before use, so seg_crc / seg_len are read at indices < nseg only, first is read for exactly count + 1
// elements and out is written for exactly count, whatever first[] holds.  No scratch, no atomics, one launch.
//
// A wavefront owns concat::kWaveBlocks consecutive blocks; lane l < kWaveBlocks reads block l's run.  Runs of up to
// concat::kShortMax segments are folded by their lane (one product per segment).  The wavefront then takes its longer
// runs one at a time, all 64 lanes on one run: per pass of up to concat::kPassSegs segments each lane folds one
// contiguous chunk into an affine pair (M, V) -- lanes past the end carry the identity (x^0, 0) -- and an ordered 6-level
// tree over the lanes, (M1, V1) o (M2, V2) = (M1 * M2, V1 * M2 ^ V2), leaves the pass in lane 63.  The loop over the
// long runs and over a run's passes is wave-uniform (a ballot, lane reads), so the tree's cross-lane steps -- DPP
// row_shr within a 16-lane row, lane reads above it, as in the CRC kernels' lane tree -- run in full EXEC.

// kConcatThreads, kConcatWaves and the grid (concat::grid_for): concat_run.h

// X(n) = x^(8n) mod P over the set bits of n only: bit k of n < 2^61 is x^(2^(k + 3)) = x2n[k + 3]; the top three bits,
// whose 8n leaves 64 bits, are raised as x^(2^k) and squared three times (exact for every n, unlike gf2_shift's n << 3).
__device__ __forceinline__ uint32_t concat_xpow8(const uint32_t* x2n, uint64_t n) {
  uint32_t p = concat::kOne;
  for (uint64_t lo = n & ((1ull << 61) - 1); lo; lo &= lo - 1) {
    const uint32_t t = x2n[__builtin_ctzll(lo) + 3];
    p = p == concat::kOne ? t : gf2_mulmod(p, t);
  }
  const uint32_t hi = uint32_t(n >> 61);
  if (hi) {
    uint32_t q = concat::kOne;
    for (int k = 0; k < 3; ++k)
      if ((hi >> k) & 1u) q = gf2_mulmod(q, x2n[61 + k]);
    for (int k = 0; k < 3; ++k) q = gf2_mulmod(q, q);
    p = gf2_mulmod(p, q);
  }
  return p;
}

struct ConcatMul {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return gf2_mulmod(a, b); }
};

__device__ __forceinline__ uint64_t concat_readlane64(uint64_t v, int src) {
  return (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), src))) << 32) |
         uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), src));
}

// The pair of lane - 2^level for the lanes that join at `level` (concat::tree_partner); other lanes get anything.
template <int kLevel>
__device__ __forceinline__ uint32_t concat_tree_pull(uint32_t v, uint32_t lane) {
  if constexpr (kLevel == 0) return row_shr<1>(v);
  else if constexpr (kLevel == 1) return row_shr<2>(v);
  else if constexpr (kLevel == 2) return row_shr<4>(v);
  else if constexpr (kLevel == 3) return row_shr<8>(v);
  else if constexpr (kLevel == 4) {  // lanes 31 and 63 join lanes 15 and 47
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(v), 15));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(v), 47));
    return lane < 32 ? lo : hi;
  } else {  // lane 63 joins lane 31
    return uint32_t(__builtin_amdgcn_readlane(int(v), 31));
  }
}

template <int kLevel>
__device__ __forceinline__ void concat_tree_level(concat::Pair& p, uint32_t lane) {
  const concat::Pair left{concat_tree_pull<kLevel>(p.m, lane), concat_tree_pull<kLevel>(p.v, lane)};
  const concat::Pair joined = concat::compose(left, p, ConcatMul());  // every lane computes: full EXEC, no branch
  if (concat::tree_joins(lane, kLevel)) p = joined;
}

__global__ void __launch_bounds__(kConcatThreads)
crc32c_concat_kernel(const uint32_t* seg_crc, const uint64_t* seg_len,
                     const uint64_t* first, const uint32_t* init, uint32_t* out,
                     uint64_t count, uint64_t nseg, const DevTables* tabs) {
  __shared__ uint32_t x2n[64];
  if (threadIdx.x < 64) x2n[threadIdx.x] = tabs->x2n[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = uint64_t(blockIdx.x) * kConcatWaves + (threadIdx.x >> 6);
  const uint64_t b = wave * concat::kWaveBlocks + lane;
  const bool own = lane < concat::kWaveBlocks && b < count;
  concat::Run r{0, 0};
  uint32_t acc = 0;
  if (own) {
    r = concat::clamp_run(first[b], first[b + 1], nseg);
    if (init) acc = init[b];
  }
  const bool is_long = own && !concat::is_short(r);
  if (own && !is_long) {
    for (uint64_t j = r.s; j < r.e; ++j) acc = gf2_mulmod(acc, concat_xpow8(x2n, seg_len[j])) ^ seg_crc[j];
    out[b] = acc;
  }
  // the longer runs of this wavefront's blocks, one at a time on all 64 lanes (wave-uniform from here on)
  for (uint64_t todo = __builtin_amdgcn_ballot_w64(is_long); todo; todo &= todo - 1) {
    const int src = __builtin_ctzll(todo);
    const uint64_t e = concat_readlane64(r.e, src);
    uint32_t run_acc = uint32_t(__builtin_amdgcn_readlane(int(acc), src));
    for (uint64_t ps = concat_readlane64(r.s, src); ps < e;) {
      const uint64_t pe = concat::pass_end(ps, e);
      const concat::Run mine = concat::lane_range(ps, pe, concat::lane_chunk(pe - ps), lane);
      concat::Pair p = concat::identity();
      for (uint64_t j = mine.s; j < mine.e; ++j)
        p = concat::compose(p, concat::Pair{concat_xpow8(x2n, seg_len[j]), seg_crc[j]}, ConcatMul());
      concat_tree_level<0>(p, lane);
      concat_tree_level<1>(p, lane);
      concat_tree_level<2>(p, lane);
      concat_tree_level<3>(p, lane);
      concat_tree_level<4>(p, lane);
      concat_tree_level<5>(p, lane);
      const uint32_t m = uint32_t(__builtin_amdgcn_readlane(int(p.m), 63));
      const uint32_t v = uint32_t(__builtin_amdgcn_readlane(int(p.v), 63));
      run_acc = gf2_mulmod(run_acc, m) ^ v;
      ps = pe;
    }
    if (lane == uint32_t(src)) out[wave * concat::kWaveBlocks + uint32_t(src)] = run_acc;
  }
}
