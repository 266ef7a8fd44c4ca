// crc32c_offsets.inc -- the offsets pass (included once, inside namespace kvsep, by crc32c_device.hip): where each kept
// block of a batch lands when the kept blocks are laid back to back, computed on the device from a verdict that is on
// the device -- the ok[] bytes of a list form, or the first_bad word of a verify call -- so that check, choose, lay out
// and copy run on one stream with no host step (DESIGN.md §3.7).
//
//   dst_off[i] = start + sum over kept k < i of (head + size_k + tail),   size_k = the sum of block k's run of seg_len,
//   dst_off[i] = kSkip for a dropped block,  *end = start + the sum over all kept blocks,  *nkept = how many are kept.
//
// An ordered exclusive scan in three kernels, ordered by the stream alone as the verdict pass (crc32c_verdicts.inc): no
// atomics, no look-back, no workgroup waits for another, and every word a replay reads was written by that replay.
//
//   offsets_tile_sum_kernel   one workgroup per tile of offsets::kTile blocks, a lane owns a block per row: the kept
//                             blocks' runs are summed (a run over concat::kShortMax segments by the whole wavefront,
//                             one at a time, in a wave-uniform loop), the extents go to ext[], the tile's total and
//                             its number of kept blocks to tile_sum[] / tile_kept[].
//   offsets_tile_scan_kernel  one workgroup: exclusive prefix sum of the tile totals (each thread a contiguous run of
//                             tiles, the 256 run sums scanned in LDS) into tile_base[]; the grand totals into grand[2].
//   offsets_write_kernel      one workgroup per tile again: an inclusive wave scan of the extents per row (DPP row_shr
//                             within a 16-lane row, lane reads above it, full EXEC), rows chained, waves chained through
//                             LDS; dst_off[i] from the tile's base; workgroup 0 writes *end and *nkept.
//
// Every index and arithmetic decision comes from offsets_run.h, which tests/cpp/offsets_run_test.cc runs lane by lane on
// the CPU.  All sums saturate at 2^64 - 1; a kept block whose end saturates gets kSkip, and so does every kept block
// after it.  Memory touched: seg_len at indices < nseg only (first[] is clamped), and only for kept blocks; first for
// count + 1 elements; keep for count; *keep_before once per workgroup; dst_off is written for exactly count.

struct OffsetsArgs {
  const uint64_t* seg_len;
  const uint64_t* first;                  // null: block i is segment i
  const uint8_t* keep;                    // null: no mask
  const unsigned long long* keep_before;  // null: no bound
  uint64_t head, tail, start;
  uint64_t max_size;  // a block over this many bytes cannot be framed (offsets::block_size)
  uint64_t count, nseg;
  unsigned long long* ext;        // scratch: the extent of every block
  unsigned long long* tile_sum;   // scratch: per tile, the sum of its extents ...
  unsigned long long* tile_kept;  // ... and its number of kept blocks
  unsigned long long* tile_base;  // scratch: the exclusive prefix sum of tile_sum
  unsigned long long* grand;      // scratch: [total of the extents, number of kept blocks]
  uint64_t* dst_off;
  uint64_t* end;
  uint64_t* nkept;  // nullable
};

template <int N>
__device__ __forceinline__ uint64_t offsets_row_shr64(uint64_t v) {
  return (uint64_t(row_shr<N>(uint32_t(v >> 32))) << 32) | row_shr<N>(uint32_t(v));
}

template <int kStep>
__device__ __forceinline__ void offsets_scan_step(uint64_t& v, uint32_t lane) {
  constexpr uint32_t n = offsets::scan_shift(kStep);
  const uint64_t left = offsets_row_shr64<int(n)>(v);  // every lane pulls: full EXEC, no branch
  v = offsets::add_sat(v, offsets::scan_takes(lane, n) ? left : 0);
}

// The saturating inclusive scan of v over the wavefront's 64 lanes (wave-uniform call sites only).
__device__ __forceinline__ uint64_t offsets_wave_scan(uint64_t v, uint32_t lane) {
  static_assert(offsets::kScanSteps == 4, "one step per row_shr distance of a 16-lane row");
  offsets_scan_step<0>(v, lane);
  offsets_scan_step<1>(v, lane);
  offsets_scan_step<2>(v, lane);
  offsets_scan_step<3>(v, lane);
  const uint64_t t15 = concat_readlane64(v, 15), t31 = concat_readlane64(v, 31), t47 = concat_readlane64(v, 47);
  return offsets::add_sat(v, offsets::row_base(lane, t15, t31, t47));
}

__device__ __forceinline__ bool offsets_kept(const OffsetsArgs& a, uint64_t before, uint64_t i) {
  return offsets::is_kept(a.keep ? a.keep[i] : uint8_t(1), before, i);
}

__global__ void __launch_bounds__(offsets::kThreads) offsets_tile_sum_kernel(OffsetsArgs a) {
  __shared__ unsigned long long ws[offsets::kWaves];
  __shared__ uint32_t wk[offsets::kWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t before = a.keep_before ? ld_word64(a.keep_before) : offsets::kKeepAll;
  uint64_t mine = 0;
  uint32_t nk = 0;
  for (uint32_t row = 0; row < offsets::kRows; ++row) {
    const uint64_t i = offsets::block_index(blockIdx.x, w, row, lane);
    const bool own = i < a.count;
    offsets::Run r{0, 0};
    bool kept = false;
    if (own) {
      kept = offsets_kept(a, before, i);
      r = a.first ? offsets::clamp_run(a.first[i], a.first[i + 1], a.nseg) : offsets::clamp_run(i, i + 1, a.nseg);
    }
    // a dropped block adds nothing: its run is not read
    const bool is_long = kept && !offsets::is_short(r);
    uint64_t sum = 0;
    if (kept && !is_long)
      for (uint64_t j = r.s; j < r.e; ++j) sum = offsets::add_sat(sum, a.seg_len[j]);
    // the longer runs of this row, one at a time on all 64 lanes (wave-uniform from here on)
    for (uint64_t todo = __builtin_amdgcn_ballot_w64(is_long); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const offsets::Run run{concat_readlane64(r.s, src), concat_readlane64(r.e, src)};
      const uint64_t iters = offsets::long_iters(run);
      uint64_t part = 0;
      for (uint64_t k = 0; k < iters; ++k) {
        const uint64_t j = offsets::long_seg(run, k, lane);
        if (j != ~uint64_t(0)) part = offsets::add_sat(part, a.seg_len[j]);
      }
      const uint64_t total = concat_readlane64(offsets_wave_scan(part, lane), 63);
      if (lane == uint32_t(src)) sum = total;
    }
    if (own) {
      const uint64_t ext = offsets::extent(kept, a.head, offsets::block_size(sum, a.max_size), a.tail);
      a.ext[i] = ext;
      mine = offsets::add_sat(mine, ext);
    }
    nk += uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(kept)));
  }
  const uint64_t tot = concat_readlane64(offsets_wave_scan(mine, lane), 63);
  if (lane == 0) {
    ws[w] = tot;
    wk[w] = nk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0, k = 0;
    for (uint32_t v = 0; v < offsets::kWaves; ++v) {
      s = offsets::add_sat(s, ws[v]);
      k += wk[v];
    }
    a.tile_sum[blockIdx.x] = s;
    a.tile_kept[blockIdx.x] = k;
  }
}

__global__ void __launch_bounds__(offsets::kScanThreads)
offsets_tile_scan_kernel(const unsigned long long* tile_sum, const unsigned long long* tile_kept,
                         unsigned long long* tile_base, unsigned long long* grand, uint64_t ntiles) {
  __shared__ unsigned long long sh[offsets::kScanThreads], shk[offsets::kScanThreads];
  const uint32_t t = threadIdx.x;
  const offsets::Run r = offsets::scan_range(t, offsets::scan_run(ntiles), ntiles);
  unsigned long long s = 0, k = 0;
  for (uint64_t i = r.s; i < r.e; ++i) {
    s = offsets::add_sat(s, tile_sum[i]);
    k += tile_kept[i];
  }
  sh[t] = s;
  shk[t] = k;
  __syncthreads();
  for (uint32_t d = 1; d < offsets::kScanThreads; d <<= 1) {
    const unsigned long long v = t >= d ? sh[t - d] : 0, vk = t >= d ? shk[t - d] : 0;
    __syncthreads();
    sh[t] = offsets::add_sat(sh[t], v);
    shk[t] += vk;
    __syncthreads();
  }
  // the tiles before this thread's run: the inclusive sum of the thread before (no subtraction: the sums saturate)
  unsigned long long at = t ? sh[t - 1] : 0;
  const unsigned long long all = sh[offsets::kScanThreads - 1], allk = shk[offsets::kScanThreads - 1];
  for (uint64_t i = r.s; i < r.e; ++i) {
    unsigned long long v = tile_sum[i];
    // the total is in its register before the store is issued (see verdict_tile_scan_kernel)
    asm volatile("" : "+v"(v) : : "memory");
    tile_base[i] = at;
    at = offsets::add_sat(at, v);
  }
  if (t == 0) {
    grand[0] = all;
    grand[1] = allk;
  }
}

__global__ void __launch_bounds__(offsets::kThreads) offsets_write_kernel(OffsetsArgs a) {
  if (a.count == 0) {  // an empty batch: this kernel alone runs, one workgroup
    if (threadIdx.x == 0) {
      *a.end = offsets::layout_end(a.start, 0);
      if (a.nkept) *a.nkept = 0;
    }
    return;
  }
  __shared__ unsigned long long ws[offsets::kWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t before = a.keep_before ? ld_word64(a.keep_before) : offsets::kKeepAll;
  const uint64_t base = ld_word64(a.tile_base + blockIdx.x);
  uint64_t g_total = 0, g_kept = 0;
  const bool closes = blockIdx.x == 0 && threadIdx.x == 0;
  if (closes) {
    g_total = ld_word64(a.grand);
    g_kept = ld_word64(a.grand + 1);
  }
  uint64_t v[offsets::kRows], inc[offsets::kRows];
  bool kept[offsets::kRows];
#pragma unroll
  for (uint32_t row = 0; row < offsets::kRows; ++row) {
    const uint64_t i = offsets::block_index(blockIdx.x, w, row, lane);
    v[row] = 0;
    kept[row] = false;
    if (i < a.count) {
      v[row] = ld_word64(a.ext + i);
      kept[row] = offsets_kept(a, before, i);
    }
  }
  // each row's inclusive scan, then the rows before it in the wave
  uint64_t carry = 0;
#pragma unroll
  for (uint32_t row = 0; row < offsets::kRows; ++row) {
    inc[row] = offsets_wave_scan(v[row], lane);
    const uint64_t tot = concat_readlane64(inc[row], 63);
    inc[row] = offsets::add_sat(inc[row], carry);
    carry = offsets::add_sat(carry, tot);
  }
  if (lane == 0) ws[w] = carry;
  __syncthreads();
  uint64_t pre = offsets::add_sat(a.start, base);
  for (uint32_t u = 0; u < w; ++u) pre = offsets::add_sat(pre, ws[u]);
#pragma unroll
  for (uint32_t row = 0; row < offsets::kRows; ++row) {
    const uint64_t i = offsets::block_index(blockIdx.x, w, row, lane);
    if (i < a.count) a.dst_off[i] = offsets::place(kept[row], offsets::add_sat(pre, inc[row]), v[row]);
  }
  if (closes) {
    *a.end = offsets::layout_end(a.start, g_total);
    if (a.nkept) *a.nkept = g_kept;
  }
}
