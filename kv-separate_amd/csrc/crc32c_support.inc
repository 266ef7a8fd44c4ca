// crc32c_support.inc -- the small kernels around the CRC kernels (included once, inside namespace kvsep, by
// crc32c_device.hip): the combine kernel of split blocks, the piece-plan kernels, the SST trailer / verify helpers,
// the synthetic-data generator and the streaming-read ceiling kernel.

// One thread per block: Horner over the block's pieces, R <- Z_piece(R) ^ R_piece.  kVerify: also the verify form's
// compare for the split blocks (the CRC kernel checked the whole ones).  A grid of at most kCombineMaxGrid workgroups
// strides over the batch (round 6: a captured verify call keeps one verdict slot per workgroup, so the slot count is
// bounded whatever the block count).  route.h holds the constant and the grid rule.
template <bool kVerify = false>
__global__ void __launch_bounds__(256) crc32c_combine_kernel(PiecesArgs a) {
  __shared__ uint32_t zp[1024];
  for (uint32_t i = threadIdx.x; i < 1024; i += 256) zp[i] = a.zpiece[i];
  __syncthreads();
#ifdef KVSEP_DIAG  // round 6 diagnosis (tools build only): a kernel argument outside the user address range is reported
  {
    const uintptr_t p[6] = {uintptr_t(a.pstart), uintptr_t(a.partial), uintptr_t(a.out), uintptr_t(a.expect),
                            uintptr_t(a.vslot), uintptr_t(a.vslot_base)};
    for (int i = 0; i < 6; ++i)
      if (i == 5 ? a.vslot_base > 4096u : (p[i] >> 47) != 0) {
        if (threadIdx.x == 0)
          printf("KVSEP combine: wg %u arg %d = %p (pstart %p partial %p out %p expect %p vslot %p count %llu max %llu)\n",
                 blockIdx.x, i, (void*)p[i], (void*)p[0], (void*)p[1], (void*)p[2], (void*)p[3], (void*)p[4],
                 (unsigned long long)a.count, (unsigned long long)a.max_pieces);
        return;
      }
  }
#endif
  const bool fallback = a.pstart[a.count] > a.max_pieces;  // the CRC kernel ran unsplit: it emitted every block
  VAcc vacc;
  for (uint64_t b0 = uint64_t(blockIdx.x) * 256; b0 < a.count; b0 += uint64_t(gridDim.x) * 256) {
    const uint64_t b = b0 + threadIdx.x;
    const uint64_t bb = b < a.count ? b : a.count - 1;
    uint64_t s = a.pstart[bb], e = a.pstart[bb + 1];
#ifdef KVSEP_DIAG
    if (b < a.count && !fallback && (e < s || e > a.max_pieces)) {
      printf("KVSEP combine: wg %u block %llu of %llu: pieces [%llu, %llu) of %llu (pstart %p: %llx %llx .. %llx)\n",
             blockIdx.x, (unsigned long long)b, (unsigned long long)a.count, (unsigned long long)s,
             (unsigned long long)e, (unsigned long long)a.max_pieces, (void*)a.pstart,
             (unsigned long long)a.pstart[0], (unsigned long long)a.pstart[1], (unsigned long long)a.pstart[a.count]);
      s = e = 0;
    }
#endif
    // unsplit blocks (and the unsplit fallback) were emitted -- and checked -- by the CRC kernel
    const bool mine = b < a.count && e - s > 1 && !fallback;
    uint32_t crc = 0;
    if (mine) {
      uint32_t acc = a.partial[s];
      for (uint64_t g = s + 1; g < e; ++g) {
        acc = zp[acc & 255u] ^ zp[256 + ((acc >> 8) & 255u)] ^ zp[512 + ((acc >> 16) & 255u)] ^ zp[768 + (acc >> 24)];
        acc ^= a.partial[g];
      }
      crc = ~acc;
      emit_block(a, b, crc);
    }
    if (kVerify) verify_wave(vacc, mine, b0, threadIdx.x, crc, ld32(a.expect + bb));
  }
  if (kVerify) verify_publish<4, kVaccShards>(a, threadIdx.x >> 6, vacc);  // after the CRC kernel's whole-block posts
}

// The verdict of a captured verify call (PiecesArgs::vslot): the lowest bad block and the total over its n slots, one
// workgroup, stream-ordered after the kernels that wrote them.
// Start-state words written by a kernel rather than a memset node (see crc32c_plan_count_kernel): w32[0] = 0 (the
// guided counter of an unplanned batch), and the verify verdict "none" (first_bad = ~0, nbad = 0) of an empty batch.
__global__ void start_words_kernel(uint32_t* w32, unsigned long long* first_bad, unsigned long long* nbad) {
  if (threadIdx.x == 0) {
    if (w32) *w32 = 0;
    if (first_bad) *first_bad = ~0ull;
    if (nbad) *nbad = 0;
  }
}

__global__ void __launch_bounds__(256) verify_slots_reduce_kernel(const unsigned long long* vslot, uint32_t n,
                                                                  unsigned long long* first_bad,
                                                                  unsigned long long* nbad) {
  __shared__ unsigned long long sb[256], sn[256];
  unsigned long long b = ~0ull, c = 0;
#ifdef KVSEP_DIAG
  if ((uintptr_t(vslot) >> 47) || (uintptr_t(first_bad) >> 47) || (uintptr_t(nbad) >> 47) || n > 4096u) {
    if (threadIdx.x == 0) printf("KVSEP reduce: vslot %p n %u first_bad %p nbad %p\n", vslot, n, first_bad, nbad);
    return;
  }
#endif
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    const unsigned long long x = vslot[2ull * i];
    b = x < b ? x : b;
    c += vslot[2ull * i + 1];
  }
  sb[threadIdx.x] = b;
  sn[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (threadIdx.x < h) {
      const unsigned long long y = sb[threadIdx.x + h];
      sb[threadIdx.x] = y < sb[threadIdx.x] ? y : sb[threadIdx.x];
      sn[threadIdx.x] += sn[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *first_bad = sn[0] ? sb[0] : ~0ull;
    *nbad = sn[0];
  }
}

// The plan's first kernel also writes the words the rest of the call needs in their start state -- pstart[0] = 0 and
// the guided schedule's counter -- instead of two memset nodes (round 6: under capture, memset nodes of graphs
// replayed at once on several streams were seen to land with the wrong contents: pstart[0] = 0x0101010101010101,
// profiles/round6/capture_fault/; kernels stay in stream order).
__global__ void crc32c_plan_count_kernel(const uint64_t* len, uint64_t count, uint64_t piece_bytes,
                                         uint64_t* counts, uint64_t* pstart, uint32_t* counter) {
  const uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b == 0) {
    pstart[0] = 0;
    if (counter) *counter = 0;
  }
  if (b >= count) return;
  const uint64_t n = len[b];
  // floor, not ceil: piece 0 takes the remainder ON TOP of a full piece (length in [P, 2P)), so no block ends
  // up with a short remainder piece that costs a work item of its own (3b: 33-B pieces, one per record);
  // only the later pieces must be exactly P long for the combine's Z_P.
  counts[b] = n < 2 * piece_bytes ? 1u : n / piece_bytes;
}

// Verify form as a separate pass over the u32 results: only for the A/B variants of the KVSEP_DIAG tools build, whose
// kernels have no fused compare (the shipped kernels compare in place: verify_wave / verify_uniform).  Wave-level
// reduction: one atomicMin / atomicAdd per wave that saw a mismatch.
__global__ void __launch_bounds__(256) verify_finish_kernel(const uint32_t* out, const uint32_t* expect,
                                                            uint64_t count, unsigned long long* first_bad,
                                                            unsigned long long* nbad) {
  const uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool bad = b < count && mask_crc(out[b]) != expect[b];
  const uint64_t m = __builtin_amdgcn_ballot_w64(bad);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u;
  if (lane == uint32_t(__builtin_ctzll(m))) {  // the wave's first bad block is its lowest bad index
    atomicMin(first_bad, (unsigned long long)b);
    atomicAdd(nbad, (unsigned long long)__builtin_popcountll(m));
  }
}

// SST write side (table/table_builder.cc:222-225): crc = Extend(Value(block), &type, 1); trailer word = Mask(crc).
__global__ void sst_trailer_finish_kernel(const uint32_t* crc, const uint8_t* types, uint32_t* masked,
                                          uint64_t count, const DevTables* tabs) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t l = ~crc[i];
  l = tabs->byte1[(l ^ types[i]) & 0xffu] ^ (l >> 8);  // one STEP1 (util/crc32c.cc:287-292)
  masked[i] = mask_crc(~l);
}

// SST read side (table/format.cc:99-106): the block is followed by [type][Mask(crc) LE32] in the file
// image, so the check is Value(data, n + 1) against the stored word.
__global__ void sst_verify_prep_kernel(const uint8_t* base, const uint64_t* off, const uint64_t* len,
                                       uint64_t* len1, uint32_t* stored, uint64_t count) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint8_t* t = base + off[i] + len[i] + 1;
  len1[i] = len[i] + 1;
  stored[i] = uint32_t(t[0]) | (uint32_t(t[1]) << 8) | (uint32_t(t[2]) << 16) | (uint32_t(t[3]) << 24);
}

__global__ void crc32c_plan_expand_kernel(const uint64_t* pstart, uint64_t count, uint64_t max_pieces,
                                          uint32_t* pblk) {
  const uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= count) return;
  const uint64_t s = pstart[b], e = pstart[b + 1];
  for (uint64_t g = s; g < e && g < max_pieces; ++g) pblk[g] = uint32_t(b);
}

// ------------------------------------------------------------------------------------------------
// support kernels
__device__ __forceinline__ uint64_t splitmix_word(uint64_t seed, uint64_t j) {
  uint64_t z = seed + (j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Fast path: dst 16-B aligned and stream_offset % 16 == 0; each thread writes 16 B per step.
// Non-temporal stores: the data goes to HBM without staying dirty in the caches.  With plain stores the first CRC
// pass over a freshly generated batch ran ~5 % slower than the next ones (round 1's "first-pass effect", which config 5
// paid on every slice it regenerates); with nt stores the first pass runs at the later passes' rate
// (tools/cold_probe.py, retired in round 6: commit 8853f41; profiles/round3/cold_first_pass_nt.log).
__global__ void fill_splitmix_fast_kernel(uint4* dst, uint64_t n16, uint64_t seed, uint64_t w0) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n16; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t lo = splitmix_word(seed, w0 + 2 * i), hi = splitmix_word(seed, w0 + 2 * i + 1);
    const v4u v = {uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32)};
    __builtin_nontemporal_store(v, reinterpret_cast<__attribute__((address_space(1))) v4u*>(
                                       reinterpret_cast<uintptr_t>(dst + i)));
  }
}

__global__ void fill_splitmix_bytes_kernel(uint8_t* dst, uint64_t n, uint64_t seed, uint64_t so) {
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t gpos = so + i;
    dst[i] = uint8_t(splitmix_word(seed, gpos >> 3) >> (8 * (gpos & 7)));
  }
}

// The attainable-read ceiling: the fastest read-only streaming pattern of tools/hbm_probe.hip's sweeps.  Each
// 8-wave workgroup owns a contiguous 1 MiB chunk at a time and its waves read interleaved 1 KiB rows (wave w:
// rows w, w+8, ...), 8 rows in flight per wave, non-temporal loads, one workgroup per CU: 7.17-7.22 TB/s on
// 64 GiB, against 6.9-7.1 for per-wave chunks at 16 rows in flight and 6.3 for plain loads.
constexpr int kStreamRows = 8;
__global__ void __launch_bounds__(512) stream_read_kernel(uintptr_t src, uint64_t n16, uint32_t* sink) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  constexpr uint64_t kChunk16 = (1u << 20) / 16;
  constexpr uint64_t kStep = 8 * kStreamRows * kRowBytes;  // bytes per round of the workgroup
  const uint64_t nchunks = n16 / kChunk16;
  uint32_t acc = 0;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uintptr_t p = src + c * kChunk16 * 16 + uintptr_t(w) * kRowBytes + lane * 16u;
#pragma unroll 1  // one round at a time: software-pipelining rounds (16 rows in flight) measured 5 % slower
    for (uint64_t r = 0; r < kChunk16 * 16; r += kStep) {
      uint4 v[kStreamRows];
#pragma unroll
      for (int u = 0; u < kStreamRows; ++u) v[u] = ld16<true>(p + r + uint64_t(u) * 8 * kRowBytes);
#pragma unroll
      for (int u = 0; u < kStreamRows; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
  }
  const uint64_t nthreads = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t i = nchunks * kChunk16 + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n16; i += nthreads) {
    const uint4 x = ld16<true>(src + i * 16);
    acc ^= x.x ^ x.y ^ x.z ^ x.w;
  }
  if (acc == 0x9e3779b9u) atomicXor(sink, acc);  // keeps the loads live; practically never stores
}
