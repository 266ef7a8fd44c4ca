// crc32c_diag.inc -- the KVSEP_DIAG tools build (`make -C kv-separate_amd diag` -> tools/libkvsep_diag.so), included by
// crc32c_device.hip after the context struct: the A/B and ablation variants of the wide and narrow kernels -- types
// with Exact's members that replace its steps (the ablations give wrong results by design), selected per context by
// KVSEP_CRC_VARIANT / KVSEP_NARROW --, the read-pattern probe kernels and the host hooks that route to them.  In the
// shipped library only the constant-false hooks at the end are compiled: no variant type, no environment variable, no
// per-context variant state.  DESIGN.md sections 3-4 give what each variant measured.

#ifdef KVSEP_DIAG
#include <unordered_map>

namespace kvsep {
// ---- wide-kernel ablations (wrong results by design) and A/B forms, as Ext types of crc32c_pieces_kernel / finish
struct AblNoMerge : Exact {  // 8: no lane merge: the four chains' XOR is the "register"
  static constexpr bool kMerge = false;
  __device__ static __forceinline__ uint32_t unmerged(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                      uint32_t lane) {
    return c0 ^ c1 ^ c2 ^ c3 ^ lane;
  }
};
struct AblXorRows : Exact {  // 9 (wide) / 16, 17 (narrow): every fold a plain XOR
  __device__ static __forceinline__ uint32_t fold(const uint8_t*, uint32_t c, uint32_t w, uint32_t, uint32_t) {
    return c ^ w;
  }
  template <typename Lay>
  __device__ static __forceinline__ uint32_t nfold(const uint8_t*, uint32_t c, uint32_t w, uint32_t, uint32_t) {
    return c ^ w;
  }
};
struct AblNoHeadTail : Exact {  // 11: no serial head / tail bytes
  static constexpr bool kHeadTail = false;
};
struct AblNoTree : Exact {  // 12: no lane tree
  static constexpr int kTreeLevels = 0;
};
struct AblFreeShort : Exact {  // 13: items of at most one row group skip their whole chain (their loads are still used)
  static constexpr bool kShortcut = true;
  template <int kG, typename Next>
  __device__ static __forceinline__ uint32_t short_item(Staged<kG>& s, uint32_t reg, Next& next) {
    next();
    uint32_t x = reg ^ s.v.x ^ s.v.w ^ s.et.x ^ s.tc.y ^ s.hc.z;
#pragma unroll
    for (int i = 0; i < kG; ++i) x ^= s.A[i].x ^ s.A[i].y ^ s.A[i].z ^ s.A[i].w;
    return x;
  }
};
struct SerialHead : Exact {  // 26 (exact): the serial head of rounds 1-3 instead of the padded one
  static constexpr bool kPad = false;
};

// ---- the sorted-window kernel's compare variants of the round-3 bisection (tools/sorted_vin_bisect.py, DESIGN.md
// §3.5): kVIn 1 = the compare inside the emit branch as before round 2 (load expected[b], compare, atomics), 2 = only
// the load of expected[b], folded into nothing, 3 / 4 = 1 plus s_nops / a full s_waitcnt after the emit's join, 5 = 1
// with a plain store in place of the atomics, 6 = the compare in full EXEC with a ballot (the shipped verify form's
// shape).  sorted_emit runs inside the emit branch (slot-end lanes of live blocks), sorted_join after its join.
template <int kVIn>
struct SortedVIn : Exact {
  __device__ static __forceinline__ void sorted_emit(const PiecesArgs& a, uint64_t b, uint32_t reg) {
    if ((kVIn == 1 || kVIn == 3 || kVIn == 4) && a.expect && mask_crc(~reg) != a.expect[b]) {
      atomicMin(a.first_bad, (unsigned long long)b);
      atomicAdd(a.nbad, 1ull);
    }
    if (kVIn == 5 && a.expect && mask_crc(~reg) != a.expect[b]) *a.first_bad = b;  // plain store
    if (kVIn == 2 && a.expect) {
      uint32_t z = 0;
      asm volatile("" : "+v"(z));
      a.out[b] = ~reg ^ (a.expect[b] & z);
    }
  }
  __device__ static __forceinline__ void sorted_join(const PiecesArgs& a, bool mine, uint64_t w, uint32_t src,
                                                     uint32_t reg, uint32_t lane) {
    if (kVIn == 3) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // wait states after the join
    if (kVIn == 4) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (kVIn == 6 && a.expect) {  // compare with no divergent region around it: load, compare, ballot in full EXEC
      const uint64_t b = mine ? w + src : 0;
      const bool bad = mine && mask_crc(~reg) != a.expect[b];
      const uint64_t m = __builtin_amdgcn_ballot_w64(bad);
      if (m) {  // wave-uniform
        const uint32_t sl = uint32_t(__builtin_ctzll(m));
        const uint64_t fb = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b >> 32)), int(sl)))) << 32) |
                            uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b)), int(sl)));
        if (lane == 0) {
          atomicMin(a.first_bad, (unsigned long long)fb);
          atomicAdd(a.nbad, (unsigned long long)__builtin_popcountll(m));
        }
      }
    }
  }
};
struct SortedDrain : Exact {  // 23: vmcnt(0) after each group's emit
  static constexpr bool kDrain = true;
};

// Diagnostic (wrong results by design): does a read pattern keep its rate once every row goes through the CRC
// kernel's Z_1024 fold chain?  kWgChunk: the ceiling's pattern above (the workgroup's waves interleave the rows of
// one 1 MiB chunk); else per-wave contiguous 128 KiB chunks, round-robin (the CRC kernel's piece pattern).  Each lane
// folds its 16 B per row into 4 chains through the replicated LDS table, as crc32c_pieces_kernel does.
template <bool kWgChunk, int kRows>
__global__ void __launch_bounds__(512) stream_fold_kernel(uintptr_t src, uint64_t n16, uint32_t* sink,
                                                          const DevTables* tabs) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  fill_lds<512>(lds, &tabs->z1024[0][0], tabs, threadIdx.x);
  __syncthreads();
  const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  if (kWgChunk) {
    constexpr uint64_t kChunk = 1u << 20;
    constexpr uint64_t kStep = 8 * kRows * kRowBytes;
    const uint64_t nchunks = n16 * 16 / kChunk;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
      const uintptr_t p = src + c * kChunk + uintptr_t(w) * kRowBytes + lane * 16u;
#pragma unroll 1
      for (uint64_t r = 0; r < kChunk; r += kStep) {
        uint4 v[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) v[u] = ld16<true>(p + r + uint64_t(u) * 8 * kRowBytes);
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
          c0 = fold_step(lds, c0, v[u].x, lc0, lc1);
          c1 = fold_step(lds, c1, v[u].y, lc0, lc1);
          c2 = fold_step(lds, c2, v[u].z, lc0, lc1);
          c3 = fold_step(lds, c3, v[u].w, lc0, lc1);
        }
      }
    }
  } else {
    constexpr uint64_t kChunk = 128u << 10;
    const uint64_t nchunks = n16 * 16 / kChunk, nwaves = uint64_t(gridDim.x) * 8;
    for (uint64_t c = uint64_t(w) * gridDim.x + blockIdx.x; c < nchunks; c += nwaves) {
      const uintptr_t p = src + c * kChunk + lane * 16u;
#pragma unroll 1
      for (uint64_t r = 0; r < kChunk; r += kRows * kRowBytes) {
        uint4 v[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) v[u] = ld16<true>(p + r + uint64_t(u) * kRowBytes);
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
          c0 = fold_step(lds, c0, v[u].x, lc0, lc1);
          c1 = fold_step(lds, c1, v[u].y, lc0, lc1);
          c2 = fold_step(lds, c2, v[u].z, lc0, lc1);
          c3 = fold_step(lds, c3, v[u].w, lc0, lc1);
        }
      }
    }
  }
  const uint32_t acc = c0 ^ c1 ^ c2 ^ c3;
  if (acc == 0x9e3779b9u) atomicXor(sink, acc);
}

// Config 2, round 4 (VERDICT r3 next #2): dynamic 8-block groups with no returning atomic in the workers' vmcnt stream.
// Groups travel through an LDS queue: a worker wave claims the next entry with an LDS atomic (lgkmcnt, never vmcnt), so
// its row loads are never held behind a global round trip.
//   kProducer = false: the WG-local form: the workgroup's contiguous run of groups is dealt to its waves by the LDS
//     claim counter alone (no global atomics at all): waves the memory system serves first take more of the run.
//   kProducer = true: the last wave of the workgroup is a producer: it grabs groups from one of 8 partition heads (one
//     per XCD residue of blockIdx, global atomics in ITS vmcnt stream only) into an LDS ring, kDepth entries ahead of
//     the workers; the workers' first round is static (wave-major), so they start before any grab returns.  The
//     partition words reset themselves (the partition's last producer to finish), so a launch needs no memset.
// Each worker keeps the narrow kernel's pipeline: the next group's rows are staged inside the current group's finish,
// and the group after that is claimed and its descriptors loaded right after the current group's emit.  Blocks over
// the hint go to narrow_deferred after the wave's last group, from a per-wave LDS list of up to kDefer groups (walked
// inside the loop, its registers made the 16-wave kernel spill); a wave with more such groups leaves the rest
// unchecksummed -- a diag limit the parity check shows, never met by the timed batches.  Batch form only (no verify).
__device__ unsigned int g_narrow_queue[8 * 32];  // per partition (128-B lines): [0] head, [1] producers done

// kStaticRR (ablation of the WG-local form, exact): the same run dealt round-robin to the waves with no claims.
template <int kG, int kWaves, bool kProducer, bool kStaticRR = false>
__global__ void __launch_bounds__(64 * kWaves) crc32c_narrow_queue_kernel(PiecesArgs a) {
  constexpr uint32_t kThreads = 64 * kWaves, kPerGroup = 64 / kNarrowLanes, kDepth = 8, kGrab = 2;
  constexpr uint32_t kRing = kProducer ? 128 : 1;  // > kDepth + kWaves: a claimed, unread slot is never overwritten
  constexpr uint32_t kWorkers = kProducer ? kWaves - 1 : kWaves;
  constexpr uint32_t kNone = 0xffffffffu;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  __shared__ uint32_t q_ring[kRing];
  __shared__ uint32_t q_ctl[4];  // [0] entries produced, [1] claimed, [2] read
  constexpr uint32_t kDefer = 32;
  __shared__ uint32_t q_def[kWaves][kDefer];  // per wave: groups with blocks over the hint
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t j = lane & (kNarrowLanes - 1);
  const uint32_t slot = lane / kNarrowLanes;
  const uint32_t lc0 = LdsFull::lc0(lane), lc1 = LdsFull::lc1(lane);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uintptr_t dummy = reinterpret_cast<uintptr_t>(a.tabs);
  const uint64_t count = a.count;
  const uint32_t groups = uint32_t((count + kPerGroup - 1) / kPerGroup);
  const uint32_t grid = gridDim.x, b = blockIdx.x;
  const uint32_t hint32 = uint32_t(a.hint);
  // kProducer: static first round over [0, nstat), partitions over the rest
  const uint32_t nstat = kProducer ? (groups < grid * kWorkers ? groups : grid * kWorkers) : 0;
  // WG-local: this workgroup's contiguous run of groups
  const uint32_t per_wg = (groups + grid - 1) / grid;
  const uint32_t run0 = b * per_wg < groups ? b * per_wg : groups;
  const uint32_t run1 = run0 + per_wg < groups ? run0 + per_wg : groups;
  if (tid == 0) q_ctl[0] = q_ctl[1] = q_ctl[2] = 0;  // before the fill's barrier; every claim comes after it

  if (kProducer && wave == kWorkers) {  // ---- the producer wave
    fill_lds<kThreads, true>(lds, &a.tabs->znarrow[0][0], a.tabs, tid);
    __syncthreads();
    if (lane == 0) {
      const uint32_t nparts = grid < 8 ? grid : 8;  // every partition has a producer
      const uint32_t p = b % nparts, ndyn = groups - nstat, per_p = (ndyn + nparts - 1) / nparts;
      const uint32_t base_p = nstat + p * per_p;
      const uint32_t n_p = ndyn > p * per_p ? (ndyn - p * per_p < per_p ? ndyn - p * per_p : per_p) : 0;
      const uint32_t nwg_p = (grid - p + nparts - 1) / nparts;
      unsigned int* head = &g_narrow_queue[p * 32];
      uint32_t prod = 0, sentinels = 0;
      bool exhausted = n_p == 0;
      while (sentinels < kWorkers) {
        while (prod - __hip_atomic_load(&q_ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= kDepth)
          __builtin_amdgcn_s_sleep(1);
        if (!exhausted) {
          const uint32_t old = atomicAdd(head, kGrab);
          for (uint32_t k = 0; k < kGrab; ++k)
            if (old + k < n_p) q_ring[prod++ % kRing] = base_p + old + k;
          exhausted = old + kGrab >= n_p;
        } else {
          q_ring[prod++ % kRing] = kNone;
          ++sentinels;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the ring entries are in LDS before the count says so
        __hip_atomic_store(&q_ctl[0], prod, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if (atomicAdd(&head[1], 1u) + 1 == nwg_p) {  // the partition's last producer: reset for the next launch
        atomicExch(head, 0u);
        atomicExch(&head[1], 0u);
      }
    }
    return;
  }

  // ---- a worker wave.  Its first group is static (before the fill's barrier: wave-major over [0, nstat) with a
  // producer, the wave's slot of the workgroup's run without); every later one is claimed after the barrier, and once
  // a claim has returned kNone the wave claims nothing more (with a producer each worker takes exactly one of its
  // kWorkers end sentinels, so no claimed ring slot is ever left unproduced).
  bool ended = false;
  auto first_group = [&]() -> uint32_t {  // no claim: LDS counters are not set up before the barrier
    const uint32_t g = kProducer ? wave * grid + b : run0 + wave;
    return (kProducer ? g < nstat : g < run1) ? g : kNone;
  };
  uint32_t rr = wave;  // kStaticRR: this wave's position in the run
  auto next_group = [&]() -> uint32_t {
    if (ended) return kNone;
    if (kStaticRR) {
      rr += kWorkers;
      ended = run0 + rr >= run1;
      return ended ? kNone : run0 + rr;
    }
    uint32_t s = 0;
    if (lane == 0) s = atomicAdd(&q_ctl[1], 1u);
    s = uint32_t(__builtin_amdgcn_readfirstlane(int(s)));
    if (!kProducer) {
      const uint32_t g = run0 + kWorkers + s;
      ended = g >= run1;
      return ended ? kNone : g;
    }
    while (__hip_atomic_load(&q_ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= s)
      __builtin_amdgcn_s_sleep(1);
    const uint32_t g = q_ring[s % kRing];
    if (lane == 0) atomicAdd(&q_ctl[2], 1u);
    ended = g == kNone;
    return g;
  };
  struct Desc {
    uint64_t off;
    uint32_t len, lenhi, init;
  };
  auto load_desc = [&](uint32_t g, Desc& d) {
    uint32_t sl = slot;
    asm volatile("" : "+v"(sl));
    const uint64_t blk = uint64_t(g) * kPerGroup + sl;
    const bool in = g != kNone && blk < count;
    const uint64_t bb = in ? blk : 0;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);
    d.len = l.x;
    d.lenhi = l.y;
    d.init = *(a.init && in ? a.init + bb : &a.tabs->z4[0][0]);
  };
  struct QItem {
    uint32_t g, reg0, kmin, kmax;
    bool over, deferred;
  };
  Desc dn;
  auto take = [&](uint32_t g, QItem& it, NStaged<kG>& st) {
    const uint64_t blk = uint64_t(g) * kPerGroup + slot;
    const bool in = g != kNone && blk < count;
    const bool over = in && (dn.lenhi != 0 || dn.len > hint32);
    it.deferred = __builtin_amdgcn_ballot_w64(over) != 0;
    const bool live = in && !over;
    it.g = g;
    it.over = over;
    it.reg0 = ~dn.init;
    nstage<kG, true, true>(st, live ? reinterpret_cast<uintptr_t>(a.base) + dn.off : dummy, live ? dn.len : 0u, j,
                           dummy);
    uint32_t km = 0, kn = ~0u;
#pragma unroll
    for (uint32_t k = 0; k < kPerGroup; ++k) {
      const uint32_t kk = uint32_t(__builtin_amdgcn_readlane(int(st.K), int(k * kNarrowLanes)));
      km = km > kk ? km : kk;
      kn = kn < kk ? kn : kk;
    }
    it.kmax = km;
    it.kmin = kn;
  };
  uint32_t gn = kNone;  // the group staged next (its descriptors are in dn until take)
  uint32_t ndef = 0;
  auto step = [&](QItem& ia, NStaged<kG>& A, QItem& ib, NStaged<kG>& B) -> bool {
    const uint32_t reg = nfinish<kG, true, true>(lds, A, ia.reg0, j, lc0, lc1, ia.kmin, ia.kmax, dummy,
                                                 [&]() { take(gn, ib, B); });
    const uint64_t blk = uint64_t(ia.g) * kPerGroup + slot;
    if (j == kNarrowLanes - 1 && blk < count && !ia.over) emit_block(a, blk, ~reg);
    if (ia.deferred) {  // wave-uniform
      if (ndef < kDefer && lane == 0) q_def[wave][ndef] = ia.g;
      ++ndef;
    }
    gn = next_group();  // the group after ib: claimed now, its descriptors loaded while ib runs
    load_desc(gn, dn);
    return ib.g != kNone;
  };

  uint32_t g0 = first_group();
  load_desc(g0, dn);
  fill_lds<kThreads, true>(lds, &a.tabs->znarrow[0][0], a.tabs, tid);
  __syncthreads();
  if (g0 == kNone) {  // no static group: claim (with a producer, until this worker's end sentinel)
    g0 = next_group();
    load_desc(g0, dn);
  }
  if (g0 == kNone) return;
  QItem cur, nxt;
  NStaged<kG> S, T;
  take(g0, cur, S);
  gn = next_group();
  load_desc(gn, dn);
  for (;;) {
    if (!step(cur, S, nxt, T)) break;
    if (!step(nxt, T, cur, S)) break;
  }
  for (uint32_t k = 0; k < ndef && k < kDefer; ++k) {
    const uint64_t g = __hip_atomic_load(&q_def[wave][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint64_t b0 = g * kPerGroup, b1 = b0 + kPerGroup < count ? b0 + kPerGroup : count;
    VAcc none;  // batch form only
    narrow_deferred<kG, true, true>(a, lds, b0, b1, dummy, none);
  }
}
}  // namespace kvsep

namespace {
using namespace kvsep;

// The variant a context runs (set from the environment at creation), kept here so the shipped context has no such state.
struct DiagState {
  int variant = 1;  // wide-kernel variant (diag_launch_pieces), KVSEP_CRC_VARIANT
  int narrow = 1;   // narrow-kernel variant (diag_launch_narrow), KVSEP_NARROW
};
std::mutex g_diag_mu;
std::unordered_map<const kvsep_crc32c_ctx*, DiagState> g_diag;

DiagState diag_state(const kvsep_crc32c_ctx* c) {
  std::lock_guard<std::mutex> g(g_diag_mu);
  const auto it = g_diag.find(c);
  return it == g_diag.end() ? DiagState() : it->second;
}

// Wide-kernel variants (launch_pieces_v):
//   0: plain loads    2: no staging ahead    3: 8-row groups
//   5: 16-wave workgroups (the round-1 kernel)    6: 12-wave workgroups    7: 4-wave workgroups, 8-row groups
//   10: rows ending at the 16-B aligned end (before the 128-B grid)
//   22 / 24: 2- / 3-row groups
//   8, 9, 11, 12: ablations (wrong results): no lane merge, XOR folds, no head/tail steps, no tree
//   13: ablation (wrong results): items of at most one row group (K <= kG) skip their whole compute chain -- the
//       upper bound of any scheme that hides short items' LDS chains (round 4, config 4)
//   14-21: guided grabs with a fixed divisor
//   26 (exact): the serial head of rounds 1-3 (the shipped kernel pads the first chunk down to its 16-B boundary and
//       rewinds the register, round 4)
// (Round 5 dropped the measured-negative exact forms 23 / 25 -- groups folded before the next group loads, round 2 --
// and 27 / 28 -- the sweeping static deal, round 4; their code is in commit 1568471, their numbers in DESIGN.md §3.1.)
// Returns false for the shipped variant (1) and anything not listed.
template <bool P, bool D>
bool diag_launch_pieces(const kvsep_crc32c_ctx* c, unsigned grid, hipStream_t s, const PiecesArgs& a) {
  constexpr int T = kWgThreads;
  const int variant = diag_state(c).variant;
  switch (variant) {
    case 0: crc32c_pieces_kernel<P, D, 4, false, true, T><<<grid, T, 0, s>>>(a); break;
    case 2: crc32c_pieces_kernel<P, D, 4, true, false, T><<<grid, T, 0, s>>>(a); break;
    case 3: crc32c_pieces_kernel<P, D, 8, true, true, T><<<grid, T, 0, s>>>(a); break;
    case 5: crc32c_pieces_kernel<P, D, 4, true, true, 1024><<<grid, 1024, 0, s>>>(a); break;
    case 6: crc32c_pieces_kernel<P, D, 4, true, true, 768><<<grid, 768, 0, s>>>(a); break;
    case 7: crc32c_pieces_kernel<P, D, 8, true, true, 256><<<grid, 256, 0, s>>>(a); break;
    case 8: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, AblNoMerge><<<grid, T, 0, s>>>(a); break;
    case 9: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, AblXorRows><<<grid, T, 0, s>>>(a); break;
    case 10: crc32c_pieces_kernel<P, D, 4, true, true, T, false><<<grid, T, 0, s>>>(a); break;  // 16-B rows
    case 11: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, AblNoHeadTail><<<grid, T, 0, s>>>(a); break;
    case 12: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, AblNoTree><<<grid, T, 0, s>>>(a); break;
    case 13: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, AblFreeShort><<<grid, T, 0, s>>>(a); break;
    case 22: crc32c_pieces_kernel<P, D, 2, true, true, T><<<grid, T, 0, s>>>(a); break;  // 2-row groups
    case 24: crc32c_pieces_kernel<P, D, 3, true, true, T><<<grid, T, 0, s>>>(a); break;  // 3-row groups
    case 26: crc32c_pieces_kernel<P, D, 4, true, true, T, true, false, SerialHead><<<grid, T, 0, s>>>(a); break;
    case 14:  // guided grabs of remaining / (d nwaves), d = 1, 2, 8, 16, 32, 4 (default: adaptive)
    case 15:
    case 17:
    case 18:
    case 19:
    case 20:  // divisor 4 (the fixed divisor before the adaptive one)
    case 21: {  // divisor 4, at most 64 items per grab
      PiecesArgs b = a;
      b.guided_div = variant == 14 ? 1 : variant == 15 ? 2 : variant == 17 ? 8 : variant == 18 ? 16 : variant == 19 ? 32
                     : 4;
      b.guided_cap = variant == 21 ? 64 : 0;
      crc32c_pieces_kernel<P, D, 4, true, true, T><<<grid, T, 0, s>>>(b);
      break;
    }
    default: return false;
  }
  return true;
}

// Narrow-kernel variants (KVSEP_NARROW), in place of the route's form: returns false when the route names none --
// the shipped rule, or a shipped form's own number (route.h: 6, 9, 10, 11, 20).  A number not listed runs the 16-wave
// narrow kernel's batch form, as it always has.
bool diag_launch_narrow(const route::Route& r, unsigned grid, hipStream_t s, const PiecesArgs& a) {
  const int nv = r.variant;
  const uint64_t count = a.count;
  if (nv == route::kDiagNone) return false;
  switch (nv) {
    case 2: crc32c_narrow_kernel<4, true, 512><<<grid, 512, 0, s>>>(a); break;
    case 3: crc32c_narrow_kernel<4, true, 768><<<grid, 768, 0, s>>>(a); break;
    case 4: crc32c_narrow_kernel<8, true, 512><<<grid, 512, 0, s>>>(a); break;
    case 5: crc32c_narrow_kernel<8, true, 768><<<grid, 768, 0, s>>>(a); break;
    case 12: crc32c_narrow_kernel<8, true, 512, true><<<grid, 512, 0, s>>>(a); break;
    case 14: crc32c_narrow_kernel<4, true, 1024, true><<<grid, 1024, 0, s>>>(a); break;
    case 16:  // ablation
      crc32c_narrow_kernel<4, true, 1024, false, true, LdsFull, false, AblXorRows><<<grid, 1024, 0, s>>>(a);
      break;
    case 18: crc32c_narrow_kernel<4, true, 1024, false, false><<<grid, 1024, 0, s>>>(a); break;  // 16-B rows
    case 19: crc32c_narrow_kernel<4, true, 512, true, false><<<grid, 512, 0, s>>>(a); break;     // 16-B rows
    case 17: crc32c_narrow_kernel<4, true, 512, true, true, LdsFull, false, AblXorRows><<<grid, 512, 0, s>>>(a); break;
    case 21: crc32c_narrow_sorted_kernel<4, true, 512><<<grid, 512, 0, s>>>(a); break;
    case 22: crc32c_narrow_sorted_kernel<4, true, 768><<<grid, 768, 0, s>>>(a); break;
    case 23: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedDrain><<<grid, 1024, 0, s>>>(a); break;
    case 24: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<1>><<<grid, 1024, 0, s>>>(a); break;
    case 25: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<2>><<<grid, 1024, 0, s>>>(a); break;
    case 26: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<3>><<<grid, 1024, 0, s>>>(a); break;
    case 27: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<4>><<<grid, 1024, 0, s>>>(a); break;
    case 28: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<5>><<<grid, 1024, 0, s>>>(a); break;
    case 29: crc32c_narrow_sorted_kernel<4, true, 1024, false, SortedVIn<6>><<<grid, 1024, 0, s>>>(a); break;
    // compact 80 KiB LDS image (two workgroups per CU): 30 / 34: 8-wave workgroups, two per CU, persistent (34:
    // fill overlapped); 31 / 35: one 8-block group per wave, grid over the whole batch (the dispatcher balances);
    // 32: two groups per wave; 33: 16-wave workgroups, one per CU (the conflict cost alone)
    case 30:
    case 31:
    case 32:
    case 34:
    case 35: {
      const uint64_t groups = (count + 7) / 8;
      const uint64_t per = nv == 31 || nv == 35 ? 8 : nv == 32 ? 16 : 0;
      uint64_t g2 = 2ull * grid;
      if (per && (groups + per - 1) / per > g2) g2 = (groups + per - 1) / per;
      if (nv == 34 || nv == 35)
        crc32c_narrow_kernel<4, true, 512, true, true, LdsCompact><<<unsigned(g2), 512, 0, s>>>(a);
      else
        crc32c_narrow_kernel<4, true, 512, false, true, LdsCompact><<<unsigned(g2), 512, 0, s>>>(a);
      break;
    }
    case 33: crc32c_narrow_kernel<4, true, 1024, false, true, LdsCompact><<<grid, 1024, 0, s>>>(a); break;
    case 36: crc32c_narrow_kernel<2, true, 1024, false, true, LdsCompact><<<grid, 1024, 0, s>>>(a); break;
    case 37: crc32c_narrow_kernel<2, true, 1024><<<grid, 1024, 0, s>>>(a); break;
    case 38: crc32c_narrow_kernel<4, true, 1024, true, true, LdsCompact><<<grid, 1024, 0, s>>>(a); break;
    // one wave per SIMD with deep row groups (no issue-age order between a SIMD's waves): 40 / 41: 4 waves, 16 /
    // 8-row groups; 42: 4 waves, 16-row groups, fill overlapped (8 waves with 16-row groups spill)
    case 40: crc32c_narrow_kernel<16, true, 256><<<grid, 256, 0, s>>>(a); break;
    case 41: crc32c_narrow_kernel<8, true, 256><<<grid, 256, 0, s>>>(a); break;
    case 42: crc32c_narrow_kernel<16, true, 256, true><<<grid, 256, 0, s>>>(a); break;
    // round 4, LDS-queued dynamic groups (crc32c_narrow_queue_kernel): 50 / 52: the workgroup's run dealt by an LDS
    // claim counter, 16 / 8 waves; 51 / 53: a producer wave per workgroup feeding an LDS ring from 8 partition heads,
    // 15 + 1 / 7 + 1 waves
    case 50: crc32c_narrow_queue_kernel<4, 16, false><<<grid, 1024, 0, s>>>(a); break;
    case 51: crc32c_narrow_queue_kernel<4, 16, true><<<grid, 1024, 0, s>>>(a); break;
    case 52: crc32c_narrow_queue_kernel<4, 8, false><<<grid, 512, 0, s>>>(a); break;
    case 53: crc32c_narrow_queue_kernel<4, 8, true><<<grid, 512, 0, s>>>(a); break;
    case 54: crc32c_narrow_queue_kernel<4, 8, false, true><<<grid, 512, 0, s>>>(a); break;    // 52 without claims
    case 55: crc32c_narrow_queue_kernel<4, 16, false, true><<<grid, 1024, 0, s>>>(a); break;  // 50 without claims
    // round 4, the shipped claim kernel (form 10: 4-row groups, 8 waves, 163 VGPRs) at other shapes: 56: 12 waves
    // (163 VGPRs fit 3 waves per SIMD); 57: 8-row groups (227 VGPRs); 59: the first group's rows staged after the LDS
    // fill (before round 4's last change).  16 waves spill even with 2-row groups.
    case 56: crc32c_narrow_claim_kernel<4, 768><<<grid, 768, 0, s>>>(a); break;
    case 57: crc32c_narrow_claim_kernel<8, 512><<<grid, 512, 0, s>>>(a); break;
    case 59: crc32c_narrow_claim_kernel<4, 512, false, false><<<grid, 512, 0, s>>>(a); break;  // no fill overlap
    case 60: crc32c_narrow_claim_kernel<4, 512, false, true, 16><<<grid, 512, 0, s>>>(a); break;  // 4-block groups
    // round 6: the claim kernel with VERDICT r5's levers (kLean): 61 the fill fetching each table entry once, 62 no
    // head / tail loads for groups without such chunks, 63 both (= the shipped form 10 since round 6), 64 both and no
    // init load for init-less batches; 65 neither (the round-5 form 10)
    case 61: crc32c_narrow_claim_kernel<4, 512, false, true, 8, 1><<<grid, 512, 0, s>>>(a); break;
    case 62: crc32c_narrow_claim_kernel<4, 512, false, true, 8, 2><<<grid, 512, 0, s>>>(a); break;
    case 63: crc32c_narrow_claim_kernel<4, 512, false, true, 8, 3><<<grid, 512, 0, s>>>(a); break;
    case 64: crc32c_narrow_claim_kernel<4, 512, false, true, 8, 7><<<grid, 512, 0, s>>>(a); break;
    case 65: crc32c_narrow_claim_kernel<4, 512><<<grid, 512, 0, s>>>(a); break;  // the round-5 form (kLean 0)
    default: crc32c_narrow_kernel<4, true, 1024><<<grid, 1024, 0, s>>>(a); break;
  }
  return true;
}

// the host hooks of crc32c_device.hip
void diag_env(kvsep_crc32c_ctx* c) {
  DiagState d;
  if (const char* v = std::getenv("KVSEP_CRC_VARIANT")) d.variant = std::atoi(v);
  if (const char* v = std::getenv("KVSEP_NARROW")) d.narrow = std::atoi(v);
  if (const char* v = std::getenv("KVSEP_CRC_STATIC_RR")) c->static_contig = std::atoi(v) ? 0 : 1;
  std::lock_guard<std::mutex> g(g_diag_mu);
  g_diag[c] = d;
}

void diag_forget(const kvsep_crc32c_ctx* c) {
  std::lock_guard<std::mutex> g(g_diag_mu);
  g_diag.erase(c);
}

// KVSEP_NARROW, as route::decide takes it (route.h: 0 never narrow, 1 / 7 the shipped rule, a shipped form's number
// that form, the rest the variants above).  Narrow variants: 2: always 8 waves; 3: 12 waves; 4 / 5: 8-row groups at
// 8 / 12 waves; 6: always 16 waves; 9: 8 waves, fill overlapped with the first loads; 20 / 21 / 22: sorted windows at
// 16 / 8 / 12 waves; the rest above
int diag_narrow(const kvsep_crc32c_ctx* c) { return diag_state(c).narrow; }

// the sorted-window variants that post first_bad / nbad themselves (kVIn 1, 3, 4, 6: compare + atomics); 25 (load
// only) and 28 (a plain store of first_bad, no count) do not, so the verify call runs verify_finish_kernel for them
bool diag_self_compare(int nv) { return nv == 24 || nv == 26 || nv == 27 || nv == 29; }

// A verify call on a narrow variant: the variants post to the caller's words directly, captured or not, from their own
// in-kernel compare or from verify_finish_kernel, so those words are set first and the call takes no verdict slots.
// (These two memset nodes are the tools build's alone: no shipped route reaches them.)
hipError_t diag_verify_words(const route::Route& r, hipStream_t s, PiecesArgs& a) {
  if (r.variant == route::kDiagNone || !a.expect) return hipSuccess;
  a.vslot = nullptr;
  const hipError_t e = hipMemsetAsync(a.first_bad, 0xff, 8, s);
  return e != hipSuccess ? e : hipMemsetAsync(a.nbad, 0, 8, s);
}

// ... and the separate compare pass for the variants that have none of their own
hipError_t diag_verify_finish(const route::Route& r, hipStream_t s, const PiecesArgs& a) {
  if (r.variant == route::kDiagNone || !a.expect || diag_self_compare(r.variant)) return hipSuccess;
  verify_finish_kernel<<<unsigned((a.count + 255) / 256), 256, 0, s>>>(a.out, a.expect, a.count, a.first_bad, a.nbad);
  return hipGetLastError();
}

// KVSEP_CRC_VARIANT 31-34: the read patterns with the fold chain (stream_fold_kernel) in place of the ceiling
bool diag_stream_read(const kvsep_crc32c_ctx* c, hipStream_t s, uintptr_t sp, uint64_t n16, uint32_t* sink) {
  const unsigned g = unsigned(c->num_cus);
  switch (diag_state(c).variant) {
    case 31: stream_fold_kernel<true, 8><<<g, 512, 0, s>>>(sp, n16, sink, c->d_tabs); return true;
    case 32: stream_fold_kernel<true, 4><<<g, 512, 0, s>>>(sp, n16, sink, c->d_tabs); return true;
    case 33: stream_fold_kernel<false, 8><<<g, 512, 0, s>>>(sp, n16, sink, c->d_tabs); return true;
    case 34: stream_fold_kernel<false, 4><<<g, 512, 0, s>>>(sp, n16, sink, c->d_tabs); return true;
    default: return false;
  }
}
}  // namespace

#else  // the shipped library: every hook is a constant

namespace {
inline void diag_env(kvsep_crc32c_ctx*) {}
inline void diag_forget(const kvsep_crc32c_ctx*) {}
inline int diag_narrow(const kvsep_crc32c_ctx*) { return kvsep::route::kDiagNone; }
inline hipError_t diag_verify_words(const kvsep::route::Route&, hipStream_t, kvsep::PiecesArgs&) { return hipSuccess; }
inline hipError_t diag_verify_finish(const kvsep::route::Route&, hipStream_t, const kvsep::PiecesArgs&) { return hipSuccess; }
inline bool diag_stream_read(const kvsep_crc32c_ctx*, hipStream_t, uintptr_t, uint64_t, uint32_t*) { return false; }
template <bool P, bool D>
inline bool diag_launch_pieces(const kvsep_crc32c_ctx*, unsigned, hipStream_t, const kvsep::PiecesArgs&) {
  return false;
}
inline bool diag_launch_narrow(const kvsep::route::Route&, unsigned, hipStream_t, const kvsep::PiecesArgs&) { return false; }
}  // namespace

#endif  // KVSEP_DIAG
