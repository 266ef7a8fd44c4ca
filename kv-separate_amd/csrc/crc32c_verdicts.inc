// crc32c_verdicts.inc -- the list pass of the verify forms (included once, inside namespace kvsep, by
// crc32c_device.hip): which blocks mismatch, as an ascending index list and / or one verdict byte per block.
//
// It runs after a verify call, on the CRCs that call just wrote (out[]) and the stored words it compared them with:
// the fused compare of the CRC kernels keeps only the lowest bad block and a count (DESIGN.md §3.4).  An ordered
// stream compaction in three kernels, ordered by the stream alone -- no workgroup waits for another:
//
//   verdict_tile_count_kernel   one workgroup per tile of kListTile blocks: bad = Mask(out[i]) != stored[i] per lane,
//                               a ballot per 64-block row, popcounts summed into the tile's total; writes ok[] when
//                               the caller wants it.
//   verdict_tile_scan_kernel    one workgroup: exclusive prefix sum of the tile totals (each thread a contiguous run of
//                               tiles, the 256 run sums scanned in LDS).
//   verdict_scatter_kernel      one workgroup per tile again: the ballots once more (8 B per block, from L2), each bad
//                               lane's position = tile base + earlier waves + earlier rows + mbcnt of its row's ballot;
//                               positions >= bad_cap are dropped.
//
// The verify call has published *nbad before these kernels start (stream order).  On a clean batch every kernel
// returns after that one load (the count kernel only when no ok[] is wanted), so nothing reads the tile arrays: a
// replay never reads a word it did not write.

// kListTile (1024 blocks: 4 waves x 4 rows of 64), kListRows and kListThreads: offsets_run.h

__device__ __forceinline__ unsigned long long ld_word64(const unsigned long long* p) {
  return *reinterpret_cast<const __attribute__((address_space(1))) unsigned long long*>(reinterpret_cast<uintptr_t>(p));
}

// The ballots of one wave's rows: row j covers blocks i0 + 64 j + lane.  Returns their popcount sum.
__device__ __forceinline__ uint32_t verdict_rows(const uint32_t* out, const uint32_t* stored, uint64_t count,
                                                 uint64_t i0, uint32_t lane, uint64_t (&m)[kListRows]) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kListRows; ++j) {
    const uint64_t i = i0 + 64u * j + lane;
    bool bad = false;
    if (i < count) bad = mask_crc(ld32(out + i)) != ld32(stored + i);
    m[j] = __builtin_amdgcn_ballot_w64(bad);
    c += uint32_t(__builtin_popcountll(m[j]));
  }
  return c;
}

// nbad null: no early return (the caller has no verdict words: kvsep_log_verify_device).  tile_cnt null: ok[] only.
__global__ void __launch_bounds__(256) verdict_tile_count_kernel(const uint32_t* out, const uint32_t* stored,
                                                                 uint64_t count, const unsigned long long* nbad,
                                                                 uint8_t* ok, uint32_t* tile_cnt) {
  if (!ok && nbad && ld_word64(nbad) == 0) return;  // a clean batch: nothing to list
  __shared__ uint32_t wc[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t i0 = uint64_t(blockIdx.x) * kListTile + w * (64u * kListRows);
  uint64_t m[kListRows];
  const uint32_t c = verdict_rows(out, stored, count, i0, lane, m);
  if (ok) {
#pragma unroll
    for (int j = 0; j < kListRows; ++j) {
      const uint64_t i = i0 + 64u * j + lane;
      if (i < count) ok[i] = uint8_t(((m[j] >> lane) & 1u) ^ 1u);
    }
  }
  if (!tile_cnt) return;
  if (lane == 0) wc[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ void __launch_bounds__(256) verdict_tile_scan_kernel(const uint32_t* tile_cnt, unsigned long long* tile_base,
                                                                uint32_t ntiles, const unsigned long long* nbad) {
  if (ld_word64(nbad) == 0) return;
  __shared__ unsigned long long sh[256];
  const uint32_t t = threadIdx.x, run = (ntiles + 255u) / 256u;
  const uint64_t b = uint64_t(t) * run, e = b + run < ntiles ? b + run : ntiles;
  unsigned long long s = 0;
  for (uint64_t k = b; k < e; ++k) s += tile_cnt[k];
  sh[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const unsigned long long v = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  unsigned long long at = sh[t] - s;  // bad blocks in the tiles before this thread's run
  for (uint64_t k = b; k < e; ++k) {
    uint32_t cnt = tile_cnt[k];
    // the count is in its register before the store is issued: no wait then has to see past a store to a load, so
    // every wait count is sound under the loads-only counter model too (tools/isa_audit.py checks both)
    asm volatile("" : "+v"(cnt) : : "memory");
    tile_base[k] = at;
    at += cnt;
  }
}

__global__ void __launch_bounds__(256) verdict_scatter_kernel(const uint32_t* out, const uint32_t* stored,
                                                              uint64_t count, const unsigned long long* nbad,
                                                              const unsigned long long* tile_base, uint64_t* bad_idx,
                                                              uint64_t bad_cap) {
  if (ld_word64(nbad) == 0) return;
  const uint64_t base = ld_word64(tile_base + blockIdx.x);
  if (base >= bad_cap) return;  // the list is full before this tile (workgroup-uniform)
  __shared__ uint32_t wc[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t i0 = uint64_t(blockIdx.x) * kListTile + w * (64u * kListRows);
  uint64_t m[kListRows];
  const uint32_t c = verdict_rows(out, stored, count, i0, lane, m);
  if (lane == 0) wc[w] = c;
  __syncthreads();
  uint64_t pos = base;
  for (uint32_t v = 0; v < w; ++v) pos += wc[v];
#pragma unroll
  for (int j = 0; j < kListRows; ++j) {
    const uint32_t before = __builtin_amdgcn_mbcnt_hi(uint32_t(m[j] >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m[j]), 0u));
    const uint64_t p = pos + before;
    if (((m[j] >> lane) & 1u) && p < bad_cap) bad_idx[p] = i0 + 64u * j + lane;
    pos += uint32_t(__builtin_popcountll(m[j]));
  }
}
