// crc32c_fold.inc -- the device-side building blocks every CRC kernel shares (included once, inside namespace kvsep,
// by crc32c_device.hip): the table image (DevTables), the kernel arguments (PiecesArgs), the replicated-table fold
// c' = w ^ Z_d(c), the wide kernel's staging and per-item finish (head, rows, chain merge, lane tree, tail), the
// verify form's compare and publish, and the LDS fill of the table image.

// ------------------------------------------------------------------------------------------------
// LDS image of one CRC workgroup (bytes).  160,768 B of the 163,840 B a gfx950 workgroup may own.
// (kWgThreads, the default CRC workgroup of 8 waves, is route.h's.)
// [0, 128 KiB): Z_1024, 4 byte-tables x 256 entries x 32 lane copies (see fold1024)
constexpr uint32_t kZ4Off = 131072;      // Z_4     (4 KiB)
constexpr uint32_t kTreeOff = 135168;    // Z_16, Z_32, Z_64, Z_128, Z_256, Z_512 (6 x 4 KiB)
constexpr uint32_t kByteOff = 159744;    // Z_1 low-byte table (1 KiB) = the STEP1 table
constexpr uint32_t kLdsBytes = 160768;
constexpr uint32_t kRowBytes = 1024;     // 64 lanes x 16 B

struct DevTables {
  uint32_t z1024[4][256];
  uint32_t z4[4][256];      // kZ4Off
  uint32_t ztree[6][4][256];// kTreeOff   (contiguous with z4 and byte1: copied to LDS as one run)
  uint32_t byte1[256];      // kByteOff
  uint32_t zpiece[4][256];  // Z_piece_bytes, used by the combine kernel
  uint32_t znarrow[4][256]; // Z_{16 kNarrowLanes}: the replicated table of the narrow kernel
  uint32_t zsmall[3][4][256];  // Z_16K, Z_32K, Z_64K: the automatic smaller pieces of small batches
  uint32_t x2n[64];         // x^(2^k) mod P (reflected): Z_n for ANY n by square-and-multiply (gf2_shift)
  uint32_t xinv[16];        // x^(-8k) mod P: Z_k^-1, a register rewound over k bytes (the padded-head variant)
};
static_assert(sizeof(DevTables) == 4096 * 13 + 1024 + 256 + 64, "table layout");
// zsmall[k] is Z_{kSmallPiece << k} (kSmallPiece: plan_size.h)

struct PiecesArgs {
  const uint8_t* base;
  const uint64_t* off;
  const uint64_t* len;
  const uint32_t* init;             // nullable -> 0
  uint32_t* out;
  uint64_t count;
  const uint64_t* pstart;           // planned mode: piece range of block b = [pstart[b], pstart[b+1]) (u64: an
                                    // understated total_bytes cannot wrap the scan, see the max_pieces fallback)
  const uint32_t* pblk;             // planned mode: block of piece g
  uint32_t* partial;                // planned mode: raw register of piece g
  uint32_t* work_counter;           // dynamic schedule
  uint64_t piece_bytes;             // of this batch (see piece_for)
  const uint32_t* zpiece;           // Z_piece_bytes as 4 byte tables (combine kernel)
  uint64_t max_pieces;              // capacity of pblk/partial
  uint32_t static_contig;           // static schedule: contiguous item ranges per wave (else round-robin)
  uint32_t guided_div;              // dynamic schedule: a grab takes remaining / (guided_div * nwaves) items;
                                    // 0: adaptive, clamp(total / (64 * nwaves), 4, 32)
  uint32_t guided_cap;              // dynamic schedule: at most this many items per grab (0: no cap)
  uint64_t hint;                    // narrow kernel: the caller's max_len hint; longer blocks are deferred (exact)
  // verify form (kVerify kernels): Mask(crc of block b) must equal expect[b] -- the check of
  // db/value_log_reader.cc:109-122 / table/format.cc:99-106.  The caller's result words first_bad (lowest mismatching
  // block, ~0 if none) and nbad are written once, by the last workgroup of the publishing kernel (verify_publish).
  const uint32_t* expect;
  unsigned long long* first_bad;
  unsigned long long* nbad;
  const DevTables* tabs;
  // The context's accumulator words, kept in their reset state between calls (layout at vacc_shard): mismatches post
  // there (atomicMin / atomicAdd); the last workgroup to arrive copies the verdict to first_bad / nbad and resets them,
  // so a verify call needs no init launch.
  unsigned long long* vacc;
  // Captured verify calls (round 6): instead of the arrival accumulators, each publishing workgroup writes its verdict
  // (lowest bad block, count) to slot vslot_base + blockIdx.x of this array with plain stores -- no atomics, no reset
  // state -- and a one-workgroup reduce kernel after the CRC / combine kernels turns the slots into first_bad / nbad.
  // A replay that overlaps another replay of the same graph writes the same words, so its verdict stays exact.
  unsigned long long* vslot;
  uint32_t vslot_base;
};

// Descriptor reads through the constant address space: wave-uniform indices then lower to scalar
// s_load (lgkmcnt), so fetching the next item's descriptors never drains the vmcnt of in-flight
// payload loads.  Descriptors are read-only for the whole launch.
template <typename T>
__device__ __forceinline__ T ldc(const T* p, uint64_t i) {
  return reinterpret_cast<const __attribute__((address_space(4))) T*>(reinterpret_cast<uintptr_t>(p))[i];
}

__device__ __forceinline__ uint32_t lds_u32(const uint8_t* lds, uint32_t byte_off) {
  return *reinterpret_cast<const uint32_t*>(lds + byte_off);
}

// Three-input XOR as ONE instruction: CDNA4's v_bitop3_b32 with truth table 0x96 (a ^ b ^ c).  hipcc
// splits a^b^c^d of four LDS results into four v_xor_b32 (interleaved with partial lgkmcnt waits), and
// the folds are issue-bound for short blocks.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Z_d through a plain (non-replicated) 4 KiB table set at byte offset t.
__device__ __forceinline__ uint32_t zmap(const uint8_t* lds, uint32_t t, uint32_t w) {
  return lds_u32(lds, t + ((w << 2) & 0x3fcu)) ^ lds_u32(lds, t + 1024u + ((w >> 6) & 0x3fcu)) ^
         lds_u32(lds, t + 2048u + ((w >> 14) & 0x3fcu)) ^ lds_u32(lds, t + 3072u + ((w >> 22) & 0x3fcu));
}

// Z_d(w) ^ x in two v_bitop3_b32.
__device__ __forceinline__ uint32_t zmap_x(const uint8_t* lds, uint32_t t, uint32_t w, uint32_t x) {
  return xor3(xor3(lds_u32(lds, t + ((w << 2) & 0x3fcu)), lds_u32(lds, t + 1024u + ((w >> 6) & 0x3fcu)), x),
              lds_u32(lds, t + 2048u + ((w >> 14) & 0x3fcu)), lds_u32(lds, t + 3072u + ((w >> 22) & 0x3fcu)));
}

// Z_1024 through the replicated tables.  Layout: byte addr = pair*64K + b*256 + half*128 + copy*4
// with table k = 2*pair + half.  v_perm_b32 picks {copy*4 | b<<8 | pair<<16} in one instruction:
//   sel byte0 = 0x00 -> lcX.byte0 (copy*4), byte1 = 0x04+k -> c.byte k, byte2 = 0x02 -> lcX.byte2 (pair),
//   byte3 = 0x0C -> 0.
__device__ __forceinline__ uint32_t fold1024(const uint8_t* lds, uint32_t c, uint32_t lc0, uint32_t lc1) {
  const uint32_t a0 = __builtin_amdgcn_perm(c, lc0, 0x0C020400u);
  const uint32_t a1 = __builtin_amdgcn_perm(c, lc0, 0x0C020500u);
  const uint32_t a2 = __builtin_amdgcn_perm(c, lc1, 0x0C020600u);
  const uint32_t a3 = __builtin_amdgcn_perm(c, lc1, 0x0C020700u);
  return lds_u32(lds, a0) ^ lds_u32(lds, a1 + 128u) ^ lds_u32(lds, a2) ^ lds_u32(lds, a3 + 128u);
}

// c' = w ^ Z(c) through the replicated table: two v_xor3_b32 for the five terms.
__device__ __forceinline__ uint32_t fold_step(const uint8_t* lds, uint32_t c, uint32_t w, uint32_t lc0, uint32_t lc1) {
  const uint32_t a0 = __builtin_amdgcn_perm(c, lc0, 0x0C020400u);
  const uint32_t a1 = __builtin_amdgcn_perm(c, lc0, 0x0C020500u);
  const uint32_t a2 = __builtin_amdgcn_perm(c, lc1, 0x0C020600u);
  const uint32_t a3 = __builtin_amdgcn_perm(c, lc1, 0x0C020700u);
  return xor3(xor3(lds_u32(lds, a0), lds_u32(lds, a1 + 128u), w), lds_u32(lds, a2), lds_u32(lds, a3 + 128u));
}

// DPP row_shr:N -- lane l receives lane l - N of its 16-lane row (a VALU op, no LDS round trip).
template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
  return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x110 + N, 0xF, 0xF, false));
}

__device__ __forceinline__ uint4 uniform4(uint4 v) {
  return make_uint4(uint32_t(__builtin_amdgcn_readfirstlane(int(v.x))), uint32_t(__builtin_amdgcn_readfirstlane(int(v.y))),
                    uint32_t(__builtin_amdgcn_readfirstlane(int(v.z))), uint32_t(__builtin_amdgcn_readfirstlane(int(v.w))));
}

// Serial steps over bytes [q0, q1) of a 16-B aligned chunk (0 <= q0 <= q1 <= 16), wave-uniform.
// Aligned whole words take one Z_4 step (util/crc32c.cc STEP4W), the rest byte steps (STEP1).
// z4 / byte: where the LDS image keeps Z_4 and the STEP1 table (the compact narrow image reads the STEP1 table as
// Z_4's byte-3 table: Z_4(b << 24) = Z_1(b), see LdsCompact).
__device__ __forceinline__ uint32_t serial16(const uint8_t* lds, uint32_t reg, uint4 ch, int q0, int q1,
                                             uint32_t z4 = kZ4Off, uint32_t byte = kByteOff) {
  const uint32_t w[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int lo = 4 * k;
    if (q0 <= lo && lo + 4 <= q1) {
      reg = zmap(lds, z4, reg ^ w[k]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pos = lo + i;
        if (pos >= q0 && pos < q1) {
          const uint32_t b = (reg ^ (w[k] >> (8 * i))) & 0xffu;
          reg = lds_u32(lds, byte + (b << 2)) ^ (reg >> 8);
        }
      }
    }
  }
  return reg;
}

// Global (not flat) address space: flat loads would tie the LDS counter to every data load.
// Streamed payload is read once: non-temporal loads (kNT) keep it from displacing anything useful and
// measured 6.2 -> 7.0 TB/s on this access pattern (kv-separate_amd/tools/hbm_probe.hip).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 gu32x4;
template <bool kNT = false>
__device__ __forceinline__ uint4 ld16(uintptr_t addr) {
  gu32x4* g = reinterpret_cast<gu32x4*>(addr);
  u32x4 v;
  if constexpr (kNT) v = __builtin_nontemporal_load(g);
  else v = *g;
  return make_uint4(v.x, v.y, v.z, v.w);
}

// A work item's loads, issued ahead of its compute so a wave can overlap the next item's HBM latency
// with the current item's serial lane merge.  All fields are wave-uniform except the vectors.
template <int kG>
struct Staged {
  uintptr_t ps, pe, hbase, h0, a1, seg;
  uint64_t K;     // body rows (0 = no body); the last row ends at ar (kAlign) or a1
  uint4 hc, tc;   // aligned 16 B around the head / the tail
  uint4 v;        // row 0; lanes with v_ok == false (front mask) use zeros instead
  uint4 A[kG];    // rows 1 .. kG (clamped to the last row)
  uint4 et;       // kAlign: the m full 16-B chunks [ar, a1) in lanes 8-m .. 7
  uint32_t m;     // kAlign: (a1 - ar) / 16, 0..7
  uintptr_t dummy;  // a valid, cache-resident device address for loads whose data is never used
  bool v_ok;
};

// Issues a FIXED set of 3 + kG loads whatever the geometry (unneeded ones read `dummy`, a valid
// device address), so the compiler can wait for exactly this item's loads with a counted vmcnt
// while the next item's loads stay in flight; masking is deferred to finish().
// kAlign: the rows end at ar = a1 rounded down to 128 B (never below h0), so every row is exactly eight 128-B
// lines and no line is requested by two rows; the m < 8 whole 16-B chunks between ar and a1 are one extra load
// (lanes 8-m .. 7) folded by a 3-level lane tree in finish().
// kPad (round 4, the shipped form): no serial head -- the body starts at the 16-B boundary at or below ps, the bytes
// before ps are zeroed in that first chunk, and the item's register enters there already rewound over them
// (x^-8k, fill_set).  A short item's head was a chain of up to 6 dependent LDS lookups ahead of its first fold.
template <int kG, bool kNT, bool kAlign = false, bool kPad = false>
__device__ __forceinline__ void stage(Staged<kG>& s, uintptr_t ps, uintptr_t pe, uint32_t lane, uintptr_t dummy,
                                      uint32_t vz) {
  s.ps = ps;
  s.pe = pe;
  s.dummy = dummy;
  s.hbase = ps & ~uintptr_t(15);
  s.h0 = kPad && ps < pe ? s.hbase : (ps + 15) & ~uintptr_t(15);
  if (s.h0 > pe) s.h0 = pe;
  s.a1 = pe & ~uintptr_t(15);
  if (s.a1 < s.h0) s.a1 = s.h0;
  uintptr_t ar = s.a1;
  if (kAlign) {
    ar = s.a1 & ~uintptr_t(127);
    if (ar < s.h0) ar = s.h0;
    s.m = uint32_t(s.a1 - ar) >> 4;
    const bool in = lane < 8 && lane + s.m >= 8;
    s.et = ld16((in ? s.a1 - 128 + uintptr_t(lane) * 16u : dummy) + vz);
  }
  s.K = ar > s.h0 ? (uint64_t(ar - s.h0) + kRowBytes - 1) / kRowBytes : 0;
  s.seg = ar - s.K * kRowBytes + uintptr_t(lane) * 16u;
  s.v_ok = s.K && s.seg >= s.h0;  // row 0 is front-masked: lanes before h0 hold zeros
  // Head and tail chunks are wave-uniform, but their addresses are offset by the opaque zero `vz` so the
  // compiler keeps them in VGPRs: a provably uniform load result is moved to SGPRs with readfirstlane
  // right here, which waits (vmcnt) for the NEXT item's first load inside the current item -- a full HBM
  // latency per item.  finish() reads them out after this item's own wait instead.
  s.hc = ld16((ps < s.h0 ? s.hbase : dummy) + vz);  // aligned 16 B holding the head (never crosses a page)
  s.tc = ld16((s.a1 < pe ? s.a1 : dummy) + vz);     // aligned 16 B holding the tail
  s.v = ld16<kNT>(s.v_ok ? s.seg : dummy);
  const uint64_t last = s.K > 1 ? s.K - 1 : 0;
#pragma unroll
  for (int i = 0; i < kG; ++i)
    s.A[i] = ld16<kNT>(last ? s.seg + (1 + i < last ? 1 + i : last) * kRowBytes : dummy);
}

// The 16-B chunk with its bytes [0, k) zeroed (k < 16).
__device__ __forceinline__ uint4 mask_low(uint4 c, uint32_t k) {
  auto m = [k](int d) -> uint32_t {
    const int lo = int(k) - 4 * d;
    return lo <= 0 ? ~0u : lo >= 4 ? 0u : (~0u << (8 * lo));
  };
  return make_uint4(c.x & m(0), c.y & m(1), c.z & m(2), c.w & m(3));
}

// The steps of the kernel templates below that the KVSEP_DIAG tools build replaces in its A/B forms and ablations
// (crc32c_diag.inc: other types with these members; the ablations give wrong results by design).  Those types exist only
// in that build: Exact is the only one the shipped library has, so no kernel it can instantiate computes anything but
// CRC-32C.
struct Exact {
  static constexpr bool kPad = true;        // the wide kernel's padded head (stage<kPad>, round 4)
  static constexpr bool kHeadTail = true;   // the wide kernel's serial head / tail bytes
  static constexpr bool kShortcut = false;  // short items run their whole chain (no short_item member needed)
  static constexpr bool kMerge = true;      // the lane merge (no unmerged member needed)
  static constexpr int kTreeLevels = 6;     // the wide kernel's lane tree: 64 lanes
  static constexpr bool kDrain = false;     // the sorted-window kernel drains nothing after a group
  // one stride-chain step c' = w ^ Z_row(c) through the LDS table: the wide kernel's Z_1024 (fold), the narrow kernels'
  // layout Lay (nfold)
  __device__ static __forceinline__ uint32_t fold(const uint8_t* lds, uint32_t c, uint32_t w, uint32_t lc0,
                                                  uint32_t lc1) {
    return fold_step(lds, c, w, lc0, lc1);
  }
  template <typename Lay>
  __device__ static __forceinline__ uint32_t nfold(const uint8_t* lds, uint32_t c, uint32_t w, uint32_t lc0,
                                                   uint32_t lc1) {
    return Lay::fold(lds, c, w, lc0, lc1);
  }
  // the sorted-window kernel's emit / join points (the round-3 bisection's compare variants live in the diag build)
  __device__ static __forceinline__ void sorted_emit(const PiecesArgs&, uint64_t, uint32_t) {}
  __device__ static __forceinline__ void sorted_join(const PiecesArgs&, bool, uint64_t, uint32_t, uint32_t, uint32_t) {}
};

// Raw CRC register after consuming the staged item [ps, pe) from register `reg` (no final inversion).
// kPad: the padded head of stage<kPad>: `reg` is the register at hbase (rewound), the first chunk's bytes before ps
// are zeroed here.
// Rows beyond the staged ones stream kG at a time, the next kG in flight during compute.
//
// `next()` stages the FOLLOWING work item's loads.  It is called once, as late as possible while still ahead
// of this item's last wait: after the last group's row loads are issued (or at once for an item with at most
// kG rows).  So (a) the main row loop runs without the next item's 28 staged VGPRs live -- that headroom
// lets the compiler keep all 16 LDS lookups of a row in flight instead of 2 -- and (b) the next item's
// loads are the most recent ones, so every wait of this item stays a counted vmcnt that leaves them in
// flight across the lane merge.
template <int kG, bool kNT, bool kAlign, bool kPad, typename Ext, typename Next>
__device__ __forceinline__ uint32_t finish(const uint8_t* lds, Staged<kG>& s, uint32_t reg, uint32_t lane,
                                           uint32_t lc0, uint32_t lc1, Next&& next) {
  if constexpr (Ext::kShortcut) {
    if (s.K <= uint64_t(kG)) return Ext::template short_item<kG>(s, reg, next);
  }
  if (s.K) {
    const uint64_t K = s.K, last = K - 1;
    if (Ext::kHeadTail && s.ps < s.h0) reg = serial16(lds, reg, uniform4(s.hc), int(s.ps - s.hbase), int(s.h0 - s.hbase));
    uint4 v = s.v_ok ? s.v : make_uint4(0, 0, 0, 0);
    if (s.seg == s.h0) {  // the head register enters as pending word at h0
      if (kPad) v = mask_low(v, uint32_t(s.ps - s.h0));
      v.x ^= reg;
    }
    uint32_t c0 = v.x, c1 = v.y, c2 = v.z, c3 = v.w;

#define KVSEP_ROW(V)                                  \
  do {                                                \
    c0 = Ext::fold(lds, c0, (V).x, lc0, lc1);         \
    c1 = Ext::fold(lds, c1, (V).y, lc0, lc1);         \
    c2 = Ext::fold(lds, c2, (V).z, lc0, lc1);         \
    c3 = Ext::fold(lds, c3, (V).w, lc0, lc1);         \
  } while (0)
// The group's loads go out before any of its compute: the scheduler would otherwise sink them below the
// first row's lookups and shorten the time they are in flight (the loop is HBM-latency bound).
#define KVSEP_LOADB(NR, CLAMP)                                                                   \
  do {                                                                                           \
    _Pragma("unroll") for (int i = 0; i < kG; ++i)                                               \
      B[i] = ld16<kNT>(s.seg + (!(CLAMP) || (NR) + i < last ? (NR) + i : last) * kRowBytes);     \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)

    uint64_t r = 1;
    for (; r + 2 * kG <= K; r += kG) {  // full group in A, another full group after it: no next item yet
      uint4 B[kG];
      KVSEP_LOADB(r + kG, false);  // rows r+kG .. r+2kG-1 <= K-1: no clamp
#pragma unroll
      for (int i = 0; i < kG; ++i) KVSEP_ROW(s.A[i]);
#pragma unroll
      for (int i = 0; i < kG; ++i) s.A[i] = B[i];
    }
    if (r + kG <= K) {  // the last full group: its successor rows load, then the next item stages
      uint4 B[kG];
      KVSEP_LOADB(r + kG, true);
      next();
#pragma unroll
      for (int i = 0; i < kG; ++i) KVSEP_ROW(s.A[i]);
#pragma unroll
      for (int i = 0; i < kG; ++i) s.A[i] = B[i];
      r += kG;
    } else {
      next();
    }
#pragma unroll
    for (int i = 0; i < kG; ++i)  // remainder rows r .. K-1, already in A
      if (r + i < K) KVSEP_ROW(s.A[i]);
#undef KVSEP_LOADB
#undef KVSEP_ROW
    if constexpr (!Ext::kMerge) return Ext::unmerged(c0, c1, c2, c3, lane);
    // lane merge: pending word at (16*lane + 12) of the last row
    uint32_t p = zmap_x(lds, kZ4Off, c0, c1);
    p = zmap_x(lds, kZ4Off, p, c2);
    p = zmap_x(lds, kZ4Off, p, c3);
    // reduction over lanes: at level j the lanes whose low j+1 bits are all ones (64 >> (j+1) of them)
    // pull the pending word of the segment 16*2^j bytes before theirs and carry it forward by 16*2^j.
    // Only those lanes touch LDS (exec-masked), which keeps the non-replicated tree tables' bank
    // conflicts small -- the tree is the LDS hot spot for short blocks.
    // The partner of an active lane l is l - 2^j: DPP row_shr for j < 4 (within a 16-lane row), lane
    // reads for j = 4, 5 -- no ds_bpermute round trips on this latency-bound chain.
#pragma unroll
    for (int j = 0; j < Ext::kTreeLevels; ++j) {
      uint32_t o;
      if (j == 0) {
        o = row_shr<1>(p);
      } else if (j == 1) {
        o = row_shr<2>(p);
      } else if (j == 2) {
        o = row_shr<4>(p);
      } else if (j == 3) {
        o = row_shr<8>(p);
      } else if (j == 4) {  // active lanes 31 and 63 need lanes 15 and 47
        const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(p), 15));
        const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(p), 47));
        o = lane < 32 ? lo : hi;
      } else {  // active lane 63 needs lane 31
        o = uint32_t(__builtin_amdgcn_readlane(int(p), 31));
      }
      const uint32_t m = (2u << j) - 1u;
      if ((lane & m) == m) p = zmap_x(lds, kTreeOff + 4096u * j, o, p);
    }
    p = uint32_t(__builtin_amdgcn_readlane(int(p), 63));  // pending word at the last row's end - 4 (uniform)
    reg = zmap(lds, kZ4Off, p);                              // register at ar (kAlign) or a1
  } else {
    next();
    if (Ext::kHeadTail && s.ps < s.h0) reg = serial16(lds, reg, uniform4(s.hc), int(s.ps - s.hbase), int(s.h0 - s.hbase));
  }
  if (kAlign && s.m) {
    // the chunks [ar, a1) right-aligned in lanes 8-m .. 7 (zeros before), the register entering at the first one;
    // per lane the STEP4W re-injection, then a 3-level tree over lanes 0..7 (Z_16, Z_32, Z_64): lane 7 ends with
    // the pending word at a1 - 4
    uint4 e = lane < 8 && lane + s.m >= 8 ? s.et : make_uint4(0, 0, 0, 0);
    if (lane + s.m == 8) {
      if (kPad && !s.K) e = mask_low(e, uint32_t(s.ps - s.h0));  // the first chunk (ar == h0)
      e.x ^= reg;
    }
    uint32_t p = zmap_x(lds, kZ4Off, e.x, e.y);
    p = zmap_x(lds, kZ4Off, p, e.z);
    p = zmap_x(lds, kZ4Off, p, e.w);
    {
      const uint32_t o = row_shr<1>(p);
      if ((lane & 1u) == 1u) p = zmap_x(lds, kTreeOff, o, p);
    }
    {
      const uint32_t o = row_shr<2>(p);
      if ((lane & 3u) == 3u) p = zmap_x(lds, kTreeOff + 4096u, o, p);
    }
    {
      const uint32_t o = row_shr<4>(p);
      if ((lane & 7u) == 7u) p = zmap_x(lds, kTreeOff + 8192u, o, p);
    }
    reg = zmap(lds, kZ4Off, uint32_t(__builtin_amdgcn_readlane(int(p), 7)));  // register at a1
  }
  if (Ext::kHeadTail && s.a1 < s.pe) {
    uint4 t = uniform4(s.tc);
    if (kPad && s.a1 == s.h0) t = mask_low(t, uint32_t(s.ps - s.h0));  // no body: the tail chunk is the first
    reg = serial16(lds, reg, t, 0, int(s.pe - s.a1));
  }
  return reg;
}

__device__ __forceinline__ uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// a * b mod P in the reflected representation (bit 31 = x^0): carry-less multiply by VALU shifts, no tables.
__device__ __forceinline__ uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int i = 31; i >= 0; --i) {
    p ^= (0u - ((a >> i) & 1u)) & b;
    b = (b >> 1) ^ (0x82F63B78u & (0u - (b & 1u)));
  }
  return p;
}

// Z_n(reg): the register advanced over n zero bytes, for any n, = reg * x^(8n) mod P (x2n[k] = x^(2^k) mod P).
// A few thousand VALU operations: only for the rare paths that need an arbitrary shift (gf2.h has the host side).
__device__ uint32_t gf2_shift(const DevTables* tabs, uint32_t reg, uint64_t n) {
  const uint64_t e = n << 3;
  uint32_t p = 0x80000000u;  // x^0
  for (int k = 0; k < 64; ++k)
    if ((e >> k) & 1u) p = gf2_mulmod(tabs->x2n[k], p);
  return gf2_mulmod(p, reg);
}

__device__ __forceinline__ void emit_block(const PiecesArgs& a, uint64_t b, uint32_t crc) { a.out[b] = crc; }

// The verify form's accumulators (PiecesArgs::vacc, u64 words, each group on a 128-B line of its own): [0] the lowest
// mismatching block (~0: none); [1] the final arrival word, (arrivals << 40) | mismatches: every mismatch count ends
// up there, so the count travels with the arrivals; and at [16 (s + 1)] the arrival word of shard s = blockIdx.x
// mod 8 (one shard per XCD: the dispatcher deals workgroups round-robin over the 8 XCDs), used by grids whose
// workgroups arrive together (verify_publish).
constexpr uint32_t kVaccShards = 8, kVaccStride = 16;  // 16 words = 128 B
constexpr unsigned long long kArrive = 1ull << 40, kCountMask = kArrive - 1;

// A workgroup that saw a mismatch waits until its lowest-block post is performed before it arrives (verify_publish);
// a clean workgroup arrives while its last result stores are still in flight.  Atomic against atomic, a completed post
// is all the order needs.  Not __threadfence(): on gfx950 that is an L2 writeback + invalidate (buffer_wbl2 /
// buffer_inv sc1), which at the end of every wave cost 130-170 us per launch (measured).
__device__ __forceinline__ void post_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The verify form's running verdict of one wave: its lowest mismatching block and its mismatch count, wave-uniform
// (scalar registers).  Round 5: a wave no longer posts each group's mismatches with global atomics as it goes (two
// atomics on one 128-B line per group, and a vmcnt(0) that drained the next group's staged rows): on an image where
// every block is bad that serialised ~16 K atomics on one line and ran 4x the clean call (217 vs 52 us, 65,536 blocks
// of 4 KiB).  The wave keeps its verdict here; the workgroup combines its waves' verdicts at the end and posts once
// (verify_publish / verify_post).
struct VAcc {
  uint64_t best = ~0ull;
  uint32_t cnt = 0;
};

// The verify form fused into the CRC kernels (db/value_log_reader.cc:109-122, table/format.cc:99-106).  Called by the
// whole wave (full EXEC) right after a group's emit: lanes with `mine` hold block b's crc and the stored word `ex`
// they loaded before the next group's staging (so waiting for it never drains those loads).  The compare itself is
// branch-free; the wave ballots the mismatches and only a mismatch enters a wave-uniform branch, which folds the
// lowest mismatching index and the count into the wave's verdict.  A per-lane branch on the compare nested inside the
// emit's divergent branch is what made the round-1 sorted-window kernel miscompute (DESIGN §3.5).  The lane's block
// is base + idx (base wave-uniform): one VGPR for the index, not a 64-bit pair.
__device__ __forceinline__ void verify_wave(VAcc& acc, bool mine, uint64_t base, uint32_t idx, uint32_t crc,
                                            uint32_t ex) {
  const uint64_t m = __builtin_amdgcn_ballot_w64(mine && mask_crc(crc) != ex);
  if (m) {  // wave-uniform
    uint32_t best = ~0u;
    for (uint64_t t = m; t; t &= t - 1) {
      const uint32_t il = uint32_t(__builtin_amdgcn_readlane(int(idx), __builtin_ctzll(t)));
      best = il < best ? il : best;
    }
    const uint64_t b = base + best;
    acc.best = b < acc.best ? b : acc.best;
    acc.cnt += uint32_t(__builtin_popcountll(m));
  }
}

// One block checked by a whole wave whose crc and stored word are wave-uniform (the wide kernel, the deferred walk).
__device__ __forceinline__ void verify_uniform(VAcc& acc, uint64_t b, uint32_t crc, uint32_t ex) {
  if (mask_crc(crc) != ex) {  // wave-uniform
    acc.best = b < acc.best ? b : acc.best;
    acc.cnt += 1;
  }
}

// The workgroup's verdict from its waves' (every wave calls it, full EXEC): each wave's lane 0 leaves its verdict in
// the workgroup's LDS slots, a barrier, then wave 0 reads them all.  Only wave 0's return value is the workgroup's.
template <uint32_t kWaves>
__device__ __forceinline__ VAcc verify_gather(const VAcc& acc, uint32_t wave, uint32_t lane) {
  __shared__ unsigned long long v_best[kWaves];
  __shared__ uint32_t v_cnt[kWaves];
  if (lane == 0) {
    v_best[wave] = acc.best;
    v_cnt[wave] = acc.cnt;
  }
  __syncthreads();  // every wave of the workgroup is done with its groups
  VAcc wg;
  if (wave == 0) {
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      const unsigned long long b = v_best[w];
      wg.best = b < wg.best ? b : wg.best;
      wg.cnt += v_cnt[w];
    }
  }
  return wg;
}

// The lane, recomputed (v_mbcnt) rather than kept live from the kernel's start: at the 16-wave kernels' 128-VGPR cap
// one more long-lived VGPR spills.
__device__ __forceinline__ uint32_t lane_id() {
  uint32_t lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  return lane;
}

// One returning device-scope atomic add by lane 0, its old value broadcast (wave-uniform).
__device__ __forceinline__ unsigned long long arrive(unsigned long long* w, unsigned long long v, uint32_t lane) {
  unsigned long long old = 0;
  if (lane == 0) old = atomicAdd(w, v);
  return (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old >> 32)), 0))) << 32) |
         uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old)), 0));
}

// The end of a publishing verify kernel (the CRC kernel of an unsplit batch, the combine kernel of a split one), every
// workgroup: the workgroup's verdict (verify_gather); if it saw mismatches, wave 0 posts its lowest index (vacc[0],
// and waits for it), then arrives with its count added to the arrival: the last workgroup to arrive copies the verdict
// to the caller's first_bad / nbad and puts the accumulators back in their reset state (~0, 0) for the next call.  So
// a verify call needs no init launch, a clean batch costs its last workgroup one atomic round trip (vacc[0] is read,
// and reset, only when something mismatched), and a batch full of bad blocks one atomicMin per workgroup.
// kShards = 8: the workgroups arrive first on their shard's word and only each shard's last on the final word.  For a
// grid whose workgroups all arrive at once (the combine kernel): 256 arrivals on ONE word queue at ~11-13 ns each
// (MI355X_MICROARCH.md fanin: 3.2-4.5 us; measured +2.7 us on the combine kernel).  The CRC kernels' workgroups end
// over several us (issue-age staircase), so they take one level: one round trip less for the last one.
// `wave`: the wave's index in the workgroup (wave-uniform, an SGPR); the lane is recomputed here (v_mbcnt) rather than
// kept live from the kernel's start: at the 16-wave kernels' 128-VGPR cap one more long-lived VGPR spills.
// The workgroup's verdict into its slot (captured calls, PiecesArgs::vslot): wave 0, lane 0, one 16-B store.
__device__ __forceinline__ void verify_slot(const PiecesArgs& a, uint32_t wave, uint32_t lane, const VAcc& wg) {
  if (wave == 0 && lane == 0) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const u64x2 v = {(unsigned long long)wg.best, (unsigned long long)wg.cnt};
    *reinterpret_cast<u64x2*>(a.vslot + 2ull * (a.vslot_base + blockIdx.x)) = v;
  }
}

template <uint32_t kWaves, uint32_t kShards = 1>
__device__ __forceinline__ void verify_publish(const PiecesArgs& a, uint32_t wave, const VAcc& acc) {
  const uint32_t lane = lane_id();
  const VAcc wg = verify_gather<kWaves>(acc, wave, lane);
  if (a.vslot) {  // a captured call: the reduce kernel publishes
    verify_slot(a, wave, lane, wg);
    return;
  }
  if (wave != 0) return;
  if (wg.cnt) {  // wave-uniform: the workgroup's lowest bad block lands before its arrival is counted
    if (lane == 0) atomicMin(a.vacc, (unsigned long long)wg.best);
    post_wait();
  }
  unsigned long long add = kArrive + wg.cnt;  // the count travels with the arrival
  uint32_t arrivals = gridDim.x;  // expected on the final word
  if (kShards > 1) {
    const uint32_t shard = blockIdx.x % kShards;
    unsigned long long* sw = a.vacc + kVaccStride * (1 + shard);
    const unsigned long long o1 = arrive(sw, add, lane);
    if ((o1 >> 40) + 1 != (gridDim.x - shard + kShards - 1) / kShards) return;  // not the shard's last
    if (lane == 0) atomicExch(sw, 0ull);  // the shard word back to its reset state
    add = kArrive + (o1 & kCountMask) + wg.cnt;  // the shard's count: its earlier workgroups' and this one's
    arrivals = gridDim.x < kShards ? gridDim.x : kShards;
  }
  const unsigned long long old = arrive(a.vacc + 1, add, lane);
  if ((old >> 40) + 1 != arrivals || lane != 0) return;  // the last workgroup of all, lane 0
  const unsigned long long nb = (old & kCountMask) + (add & kCountMask);
  atomicExch(a.vacc + 1, 0ull);  // first, so the wait for the swap's result below is a plain vmcnt(0)
  const unsigned long long fb = nb ? atomicExch(a.vacc, ~0ull) : ~0ull;
  *a.first_bad = fb;
  *a.nbad = nb;
}

// The end of a verify CRC kernel that does not publish (the wide kernel of a split batch: the combine kernel after it
// publishes): the workgroup's verdict goes to the accumulators directly -- its lowest bad block and its count on the
// final word, where the combine kernel's arrivals find them (the kernel boundary orders them).
template <uint32_t kWaves>
__device__ __forceinline__ void verify_post(const PiecesArgs& a, uint32_t wave, const VAcc& acc) {
  const uint32_t lane = lane_id();
  const VAcc wg = verify_gather<kWaves>(acc, wave, lane);
  if (a.vslot) {
    verify_slot(a, wave, lane, wg);
    return;
  }
  if (wave == 0 && wg.cnt && lane == 0) {
    atomicMin(a.vacc, (unsigned long long)wg.best);
    atomicAdd(a.vacc + 1, (unsigned long long)wg.cnt);
  }
}

// A 32-bit global load (address space 1), for the stored words of the verify form.
__device__ __forceinline__ uint32_t ld32(const uint32_t* p) {
  return *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(reinterpret_cast<uintptr_t>(p));
}

#include "crc32c_hooks.inc"  // diagnostic hook points: empty in the shipped library

// LDS image of a CRC workgroup: the replicated fold table `rep` (4 byte-tables) at [0, 128 KiB), then the
// small tables (Z_4, the tree tables, the byte table) as one contiguous run.
struct NoMid {
  __device__ void operator()() const {}
};

// `mid()` runs between the fill's global loads and its LDS stores (pinned there by sched barriers): loads it
// issues are younger than the table loads, so the stores wait for the tables only (a counted vmcnt).
// kNarrowSet: only the small tables the narrow kernel reads -- Z_4, Z_16, Z_32, Z_64 (one 16 KiB run from kZ4Off)
// and the byte table -- not Z_128 .. Z_512 (12 KiB less to load and store per workgroup).
constexpr uint32_t kSmallAll16 = (kLdsBytes - kZ4Off) / 16;                       // uint4 in the small-table run
constexpr uint32_t kSmallNarrow16 = (4 * 4096) / 16 + 1024 / 16;                  // Z_4..Z_64 + byte table
template <bool kNarrowSet>
__device__ __forceinline__ uint32_t small_index(uint32_t q) {  // uint4 index from kZ4Off (same in src and LDS)
  return !kNarrowSet || q < 1024 ? q : (kByteOff - kZ4Off) / 16 + (q - 1024);
}

// kOnce (round 6): each of the replicated table's 1,024 distinct entries is fetched once per workgroup -- lane tid
// loads entries tid * E .. tid * E + E - 1 (E = 1024 / kThreads: one 8-B load at 512 threads, coalesced over the
// wave) and writes all 8 of each entry's 16-B copies itself, the 8 stores of an entry rotated by the lane (store i of
// lane t goes to copy (i + t) mod 8), so the 8 lanes of each ds_write_b128 group still cover one whole 128-B bank row.
// Without it every lane gathers the entry of each 16-B store it makes: 16 dword loads per lane at 512 threads, every
// entry fetched 8 times (VERDICT r5: 19 of config 2's 52 extra loads per wave).
template <int kThreads = kWgThreads, bool kNarrowSet = false, bool kOnce = false, typename Mid = NoMid>
__device__ __forceinline__ void fill_lds(uint8_t* lds, const uint32_t* rep, const DevTables* tabs, uint32_t tid,
                                         Mid&& mid = Mid()) {
  // Every global load of the fill is issued before the first LDS store: one L2/HBM round trip per
  // workgroup instead of one per loop trip (the fill is a fixed cost of every launch; it dominates
  // small batches, e.g. 4 KiB-block batches of a few MiB).
  constexpr bool kByEntry = kOnce && 1024 % kThreads == 0;
  constexpr uint32_t kEnt = kByEntry ? 1024 / kThreads : 1;                            // entries per lane
  constexpr uint32_t kRep = kByEntry ? kEnt : (8192 + kThreads - 1) / kThreads;        // loads (dwords)
  constexpr uint32_t kN16 = kNarrowSet ? kSmallNarrow16 : kSmallAll16;
  constexpr uint32_t kSmall = (kN16 + kThreads - 1) / kThreads;                        // uint4 copies
  uint4* l128 = reinterpret_cast<uint4*>(lds);
  const uint4* src = reinterpret_cast<const uint4*>(&tabs->z4[0][0]);
  uint32_t v[kRep];
  uint4 w[kSmall];
  if constexpr (kByEntry) {
    const uint32_t e0 = tid * kEnt;  // table e0 >> 8, bytes (e0 & 255) .. + kEnt - 1 (rep: 4 tables of 256 words)
    if constexpr (kEnt == 2) {
      const uint2 x = *reinterpret_cast<const uint2*>(rep + e0);
      v[0] = x.x;
      v[1] = x.y;
    } else {
#pragma unroll
      for (uint32_t e = 0; e < kEnt; ++e) v[e] = rep[e0 + e];
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kRep; ++i) {
      const uint32_t q = tid + i * kThreads;  // uint4 index in the replicated image
      const uint32_t idx = q * 4, pair = idx >> 14, b = (idx >> 6) & 255u, half = (idx >> 5) & 1u;
      v[i] = q < 8192 ? rep[(2u * pair + half) * 256u + b] : 0u;
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kSmall; ++i) {
    const uint32_t q = tid + i * kThreads;
    w[i] = q < kN16 ? src[small_index<kNarrowSet>(q)] : make_uint4(0, 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
  // 16-B stores: 4 consecutive dwords of the replicated image are 4 copies of one entry
  if constexpr (kByEntry) {
    // entry (table k, byte b) fills uint4s (k >> 1) * 4096 + b * 16 + (k & 1) * 8 + [0, 8) (see fold1024's layout)
    const uint32_t e0 = tid * kEnt, k = e0 >> 8;
#pragma unroll
    for (uint32_t e = 0; e < kEnt; ++e) {
      const uint32_t q0 = (k >> 1) * 4096u + ((e0 + e) & 255u) * 16u + (k & 1u) * 8u;
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) l128[q0 + ((i + tid) & 7u)] = make_uint4(v[e], v[e], v[e], v[e]);
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kRep; ++i) {
      const uint32_t q = tid + i * kThreads;
      if (q < 8192) l128[q] = make_uint4(v[i], v[i], v[i], v[i]);
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kSmall; ++i) {
    const uint32_t q = tid + i * kThreads;
    if (q < kN16) l128[kZ4Off / 16 + small_index<kNarrowSet>(q)] = w[i];
  }
}

// LDS layouts of the narrow kernels (template parameter Lay of nfinish and the narrow kernel).
//   LdsFull: the pieces kernel's image (157 KiB; the narrow kernel fills only Z_128 replicated 32x and the small
//     tables it reads): every lookup conflict-free, one workgroup per CU.
//   LdsCompact: 80 KiB, so that two workgroups fit one CU: Z_128 replicated 16x at byte b<<8 | k<<6 | copy<<2
//     (table k, copy = lane % 16), then Z_4 and Z_16 / Z_32 / Z_64; the STEP1 table is read as Z_4's byte-3 table
//     (Z_4(b << 24) = Z_1(b): three of the four zero bytes only shift b down).  Lanes l and l + 16 of a 32-lane
//     LDS group share a copy, so a lookup is a 2-way bank conflict (4 LDS-array cycles per wave-instruction, not 2).
struct LdsFull {
  static constexpr uint32_t kBytes = kLdsBytes, kZ4 = kZ4Off, kTree = kTreeOff, kByte = kByteOff;
  static constexpr bool kCompact = false;
  static __device__ __forceinline__ uint32_t lc0(uint32_t lane) { return (lane & 31u) << 2; }
  static __device__ __forceinline__ uint32_t lc1(uint32_t lane) { return ((lane & 31u) << 2) | 0x10000u; }
  static __device__ __forceinline__ uint32_t fold(const uint8_t* lds, uint32_t c, uint32_t w, uint32_t lc0,
                                                  uint32_t lc1) {
    return fold_step(lds, c, w, lc0, lc1);
  }
};
struct LdsCompact {
  static constexpr uint32_t kBytes = 81920, kZ4 = 65536, kTree = 65536 + 4096, kByte = 65536 + 3072;
  static constexpr bool kCompact = true;
  static __device__ __forceinline__ uint32_t lc0(uint32_t lane) { return (lane & 15u) << 2; }
  static __device__ __forceinline__ uint32_t lc1(uint32_t) { return 0; }
  static __device__ __forceinline__ uint32_t fold(const uint8_t* lds, uint32_t c, uint32_t w, uint32_t lc0,
                                                  uint32_t) {
    // v_perm_b32: byte0 = lc0.byte0 (copy*4), byte1 = c.byte k, bytes 2-3 zero; table k by the immediate offset
    const uint32_t a0 = __builtin_amdgcn_perm(c, lc0, 0x0C0C0400u);
    const uint32_t a1 = __builtin_amdgcn_perm(c, lc0, 0x0C0C0500u);
    const uint32_t a2 = __builtin_amdgcn_perm(c, lc0, 0x0C0C0600u);
    const uint32_t a3 = __builtin_amdgcn_perm(c, lc0, 0x0C0C0700u);
    return xor3(xor3(lds_u32(lds, a0), lds_u32(lds, a1 + 64u), w), lds_u32(lds, a2 + 128u), lds_u32(lds, a3 + 192u));
  }
};
static_assert(LdsCompact::kTree + 3 * 4096 == LdsCompact::kBytes, "compact narrow image");

// The compact image's fill (LdsCompact): 4096 16-B stores of the replicated Z_128 and the 16 KiB run Z_4, Z_16,
// Z_32, Z_64 (contiguous in DevTables from z4).  All loads before the first store, `mid()` between (see fill_lds).
template <int kThreads, typename Mid = NoMid>
__device__ __forceinline__ void fill_lds_compact(uint8_t* lds, const uint32_t* rep, const DevTables* tabs,
                                                 uint32_t tid, Mid&& mid = Mid()) {
  constexpr uint32_t kRep = (4096 + kThreads - 1) / kThreads;
  constexpr uint32_t kN16 = 4 * 4096 / 16;
  constexpr uint32_t kSmall = (kN16 + kThreads - 1) / kThreads;
  uint4* l128 = reinterpret_cast<uint4*>(lds);
  const uint4* src = reinterpret_cast<const uint4*>(&tabs->z4[0][0]);
  uint32_t v[kRep];
  uint4 w[kSmall];
#pragma unroll
  for (uint32_t i = 0; i < kRep; ++i) {
    const uint32_t q = tid + i * kThreads;  // bytes 16q .. 16q+15 = b<<8 | k<<6 | 4 copies
    v[i] = q < 4096 ? rep[((q >> 2) & 3u) * 256u + (q >> 4)] : 0u;
  }
#pragma unroll
  for (uint32_t i = 0; i < kSmall; ++i) {
    const uint32_t q = tid + i * kThreads;
    w[i] = q < kN16 ? src[q] : make_uint4(0, 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (uint32_t i = 0; i < kRep; ++i) {
    const uint32_t q = tid + i * kThreads;
    if (q < 4096) l128[q] = make_uint4(v[i], v[i], v[i], v[i]);
  }
#pragma unroll
  for (uint32_t i = 0; i < kSmall; ++i) {
    const uint32_t q = tid + i * kThreads;
    if (q < kN16) l128[LdsCompact::kZ4 / 16 + q] = w[i];
  }
}
