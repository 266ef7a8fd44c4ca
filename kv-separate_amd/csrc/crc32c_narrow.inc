// crc32c_narrow.inc -- the narrow kernels for batches of many short blocks: 8 (or 16) lanes per block, 8 blocks per
// wavefront -- crc32c_narrow_kernel, crc32c_narrow_claim_kernel (workgroup-contiguous runs dealt by LDS claims) and
// crc32c_narrow_sorted_kernel (64-block windows sorted by length, for ragged batches).  Included once, inside
// namespace kvsep, by crc32c_device.hip; DESIGN.md §3.2-3.3.

// ------------------------------------------------------------------------------------------------
// Narrow kernel for batches of many short blocks (route::decide in route.h): a wavefront runs 8 blocks at once,
// kNarrowLanes = 8 lanes ("a slot") per block and rows of 128 B on the 128-B address grid (see nstage).  The wide
// kernel pays a fixed cost per block (lane merge, 6-level lane tree, staging: ~230 of its ~313 VALU
// instructions for a 4 KiB block, PMC SQ_INSTS_VALU); here the merge is a 3-level tree inside the slot and
// staging is shared by the 8 blocks, so the cost per block is mostly the fold itself.  The chain fold uses
// the same replicated-table lookup as the wide kernel, with Z_128 (16 B per lane x 8 lanes) in place of
// Z_1024.  All geometry is per lane (divergent across slots); every load instruction still reads whole
// 128-B lines, one per slot.
constexpr int kNarrowLanes = 8;
constexpr uint32_t kNarrowRow = 16u * kNarrowLanes;
// (kNarrowMax, the longest block these kernels are ever chosen for, and the coop form's kCoopMaxLen are route.h's.)

template <int kG>
struct NStaged {
  uintptr_t ps, seg;  // this lane's slot item [ps, ps + len); its 16-B chunk of row 0
  uint32_t len;       // < 2^31: <= the hint (<= 64 KiB) on the main path, <= 1 GiB parts on the deferred one
  uint32_t K;         // body rows of the slot item
  uint4 hc, tc, v;
  uint4 A[kG];            // rows 1 .. kG (clamped to the last row)
};

// kAlign: a slot's rows end at ar = a1 rounded down to 128 B (never below h0), so every slot row is one whole
// 128-B line; the m < 8 whole chunks [ar, a1) come in with the tail load: lane j loads a1 - 112 + 16 j, i.e.
// lanes 7-m .. 6 hold those chunks and lane 7 the partial tail chunk at a1 (the old tc) -- no extra load, no
// extra registers.  Without it a block at a 16-B but not 128-B aligned address reads two half lines per row
// (SST blocks in a file image: 20 % slower).
// The slot geometry in 32-bit offsets from the 128-B line holding ps (len < 2^31, so nothing wraps): P = ps's
// offset in that line, E = the end, h0 / a1 = the first / last 16-B boundary inside [P, E] (clamped), ar = where
// the rows end.  64-bit address arithmetic only for the loads.
struct NGeo {
  uint32_t P, E, h0, a1, ar;
};
template <bool kAlign, int kL = kNarrowLanes>
__device__ __forceinline__ NGeo ngeo(uintptr_t ps, uint32_t len) {
  constexpr uint32_t kRow = 16u * kL;
  NGeo g;
  g.P = uint32_t(ps) & (kRow - 1);
  g.E = g.P + len;
  g.h0 = (g.P + 15u) & ~15u;
  if (g.h0 > g.E) g.h0 = g.E;
  g.a1 = g.E & ~15u;
  if (g.a1 < g.h0) g.a1 = g.h0;
  g.ar = g.a1;
  if (kAlign) {
    g.ar = g.a1 & ~(kRow - 1);
    if (g.ar < g.h0) g.ar = g.h0;
  }
  return g;
}

// kSkipHT (round 6): the head and tail loads are issued only when some slot of the group has a head or tail chunk
// (a wave-uniform ballot); a group of blocks that start and end on the 128-B grid -- config 2's 4 KiB blocks, SST
// blocks of a 128-B multiple -- issues none of them (two dummy loads less per group).  The ballot makes the count of
// loads after the previous group's rows path-dependent, so a wait for those rows on a group that does load them covers
// up to two of this group's (in-order) head / tail loads as well: a few cycles, never this group's rows.
template <int kG, bool kNT, bool kAlign = true, int kL = kNarrowLanes, bool kSkipHT = false>
__device__ __forceinline__ void nstage(NStaged<kG>& s, uintptr_t ps, uint32_t len, uint32_t j, uintptr_t dummy) {
  constexpr uint32_t kRow = 16u * kL;
  s.ps = ps;
  s.len = len;
  const NGeo g = ngeo<kAlign, kL>(ps, len);
  const uintptr_t line = ps - g.P;
  s.K = (g.ar - g.h0 + kRow - 1) / kRow;
  const int32_t rel0 = int32_t(g.ar - s.K * kRow + j * 16u);  // row 0's chunk, may start before the line
  s.seg = line + intptr_t(rel0);
  const bool v_ok = s.K && rel0 >= int32_t(g.h0);
  const bool ht = !kSkipHT || __builtin_amdgcn_ballot_w64(g.P < g.h0 || g.a1 < g.E || (kAlign && g.a1 > g.ar)) != 0;
  if (ht) {
    s.hc = ld16(g.P < g.h0 ? line + (g.P & ~15u) : dummy);
    if (kAlign) {
      const uint32_t m = (g.a1 - g.ar) >> 4;
      s.tc = ld16((j == kL - 1 ? g.a1 < g.E : j + m >= kL - 1) ? line + (g.a1 - (kRow - 16u) + j * 16u) : dummy);
    } else {
      s.tc = ld16(g.a1 < g.E ? line + g.a1 : dummy);
    }
  } else {
    s.hc = s.tc = make_uint4(0, 0, 0, 0);
  }
  s.v = ld16<kNT>(v_ok ? s.seg : dummy);
  const uint32_t last = s.K > 1 ? s.K - 1 : 0;
#pragma unroll
  for (int i = 0; i < kG; ++i)
    s.A[i] = ld16<kNT>(last ? s.seg + uintptr_t(1 + i < int(last) ? 1 + i : last) * kRow : dummy);
}

// Raw register after the slot item, valid in the slot's last lane (j == 7).  kmin / kmax: wave min / max of K.
// `next()` stages the following group, after this group's last row loads (see the wide kernel's finish()).
// kL: lanes per slot, 8 (Z_128 rows, a 3-level slot tree) or 16 (diag: Z_256 rows, 4 levels; LdsFull only).
template <int kG, bool kNT, bool kAlign = true, typename Lay = LdsFull, int kL = kNarrowLanes, typename Ext = Exact,
          typename Next>
__device__ __forceinline__ uint32_t nfinish(const uint8_t* lds, NStaged<kG>& s, uint32_t reg, uint32_t j,
                                            uint32_t lc0, uint32_t lc1, uint32_t kmin, uint32_t kmax,
                                            uintptr_t dummy, Next&& next) {
  static_assert(kL == 8 || (kL == 16 && !Lay::kCompact), "slots of 8 lanes, or 16 on the full LDS image");
  constexpr uint32_t kRow = 16u * kL;
  const NGeo g = ngeo<kAlign, kL>(s.ps, s.len);
  // what the end needs, packed in one 32-bit value computed here, live across the row loop (at 16 waves the kernel
  // sits at 128 VGPRs): bits 0-3 the bytes after a1, bits 4-6 (kAlign) m, the whole chunks [ar, a1)
  const uint32_t endg = (g.E - g.a1) | (g.a1 - g.ar);
  const int32_t rel0 = int32_t(uint32_t(s.seg) - uint32_t(s.ps) + g.P);  // row 0's chunk from the line (as staged)
  if (!kmax) next();
  if (g.P < g.h0) reg = serial16(lds, reg, s.hc, int(g.P & 15u), int(g.h0 - (g.P & ~15u)), Lay::kZ4, Lay::kByte);
  if (kmax) {
    const uint32_t K = s.K, last = K > 1 ? K - 1 : 0;
    uint4 v = (K && rel0 >= int32_t(g.h0)) ? s.v : make_uint4(0, 0, 0, 0);
    if (K && rel0 == int32_t(g.h0)) v.x ^= reg;  // the head register enters as pending word at h0
    uint32_t c0 = v.x, c1 = v.y, c2 = v.z, c3 = v.w;
    KVSEP_NSTAMP_FIRST_DATA(c0);  // stamp hook (crc32c_hooks.inc): empty in the shipped library
#define KVSEP_NROW(V)                                                 \
  do {                                                                \
    c0 = Ext::template nfold<Lay>(lds, c0, (V).x, lc0, lc1);          \
    c1 = Ext::template nfold<Lay>(lds, c1, (V).y, lc0, lc1);          \
    c2 = Ext::template nfold<Lay>(lds, c2, (V).z, lc0, lc1);          \
    c3 = Ext::template nfold<Lay>(lds, c3, (V).w, lc0, lc1);          \
  } while (0)
    uint32_t r = 1;
    for (; r + 2 * kG <= kmin; r += kG) {  // every slot has rows r .. r+2kG-1: no guards, no clamps
      uint4 B[kG];
#pragma unroll
      for (int i = 0; i < kG; ++i) B[i] = ld16<kNT>(s.seg + uintptr_t(r + kG + i) * kRow);
      __builtin_amdgcn_sched_barrier(0);  // loads go out before the group's compute
#pragma unroll
      for (int i = 0; i < kG; ++i) KVSEP_NROW(s.A[i]);
#pragma unroll
      for (int i = 0; i < kG; ++i) s.A[i] = B[i];
    }
    for (; r + kG <= kmax; r += kG) {  // ragged end: per-lane clamps and guards
      uint4 B[kG];
      const uint32_t nr = r + kG;
#pragma unroll
      for (int i = 0; i < kG; ++i)
        B[i] = ld16<kNT>(last ? s.seg + uintptr_t(nr + i < last ? nr + i : last) * kRow : dummy);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < kG; ++i)
        if (r + i < K) KVSEP_NROW(s.A[i]);
#pragma unroll
      for (int i = 0; i < kG; ++i) s.A[i] = B[i];
    }
    next();
#pragma unroll
    for (int i = 0; i < kG; ++i)
      if (r + i < K) KVSEP_NROW(s.A[i]);
#undef KVSEP_NROW
    uint32_t p = zmap_x(lds, Lay::kZ4, c0, c1);
    p = zmap_x(lds, Lay::kZ4, p, c2);
    p = zmap_x(lds, Lay::kZ4, p, c3);
    // 3-level tree inside the slot (lanes 8k .. 8k+7 of one DPP row): Z_16, Z_32, Z_64
    {
      const uint32_t o = row_shr<1>(p);
      if ((j & 1u) == 1u) p = zmap_x(lds, Lay::kTree, o, p);
    }
    {
      const uint32_t o = row_shr<2>(p);
      if ((j & 3u) == 3u) p = zmap_x(lds, Lay::kTree + 4096u, o, p);
    }
    {
      const uint32_t o = row_shr<4>(p);
      if ((j & 7u) == 7u) p = zmap_x(lds, Lay::kTree + 8192u, o, p);
    }
    if (kL == 16) {  // a 16-lane slot is one DPP row: the 4th level (Z_128)
      const uint32_t o = row_shr<8>(p);
      if ((j & 15u) == 15u) p = zmap_x(lds, Lay::kTree + 12288u, o, p);
    }
    if (K) reg = zmap(lds, Lay::kZ4, p);  // lane 7 of the slot: pending word at the rows' end - 4 -> register there
  }
  if (kAlign) {
    const uint32_t m = endg >> 4;
    if (__builtin_amdgcn_ballot_w64(m != 0)) {  // whole chunks [ar, a1) in lanes 7-m .. 6 of the tail load
      // their raw register from 0: per lane the STEP4W re-injection, moved up one lane (chunks in lanes 8-m .. 7),
      // the slot's 3-level tree; then R = Z_16m(register at ar) ^ that (Z_16m from the tree tables by the bits of m)
      const uint4 e = j < kL - 1 && j + m >= kL - 1 ? s.tc : make_uint4(0, 0, 0, 0);
      uint32_t p = zmap_x(lds, Lay::kZ4, e.x, e.y);
      p = zmap_x(lds, Lay::kZ4, p, e.z);
      p = zmap_x(lds, Lay::kZ4, p, e.w);
      p = row_shr<1>(p);  // lane 8k + 7 holds no chunk (its e is zero, so p is zero): slot k+1's lane 0 gets 0
      {
        const uint32_t o = row_shr<1>(p);
        if ((j & 1u) == 1u) p = zmap_x(lds, Lay::kTree, o, p);
      }
      {
        const uint32_t o = row_shr<2>(p);
        if ((j & 3u) == 3u) p = zmap_x(lds, Lay::kTree + 4096u, o, p);
      }
      {
        const uint32_t o = row_shr<4>(p);
        if ((j & 7u) == 7u) p = zmap_x(lds, Lay::kTree + 8192u, o, p);
      }
      if (kL == 16) {
        const uint32_t o = row_shr<8>(p);
        if ((j & 15u) == 15u) p = zmap_x(lds, Lay::kTree + 12288u, o, p);
      }
      if (m & 1u) reg = zmap(lds, Lay::kTree, reg);
      if (m & 2u) reg = zmap(lds, Lay::kTree + 4096u, reg);
      if (m & 4u) reg = zmap(lds, Lay::kTree + 8192u, reg);
      if (kL == 16 && (m & 8u)) reg = zmap(lds, Lay::kTree + 12288u, reg);
      reg ^= zmap(lds, Lay::kZ4, p);  // lane 7: register at a1
    }
  }
  if (endg & 15u) reg = serial16(lds, reg, s.tc, 0, int(endg & 15u), Lay::kZ4, Lay::kByte);  // lane 7's tail load is the chunk at a1
  return reg;
}

// Blocks longer than the narrow kernel's hint (a.hint), skipped by the main pass: the wave walks its run
// [lo, hi) again and checksums those blocks one at a time, each cut into parts of <= 1 GiB, 8 at a time (one per
// slot; the slot geometry is 32-bit), merged with R(A||B) = Z_|B|(R(A)) ^ R(B) through gf2_shift.  Slower than the
// main path (long blocks are not what the narrow kernels are for) but exact for any 64-bit length.
template <int kG, bool kNT, bool kAlignN, typename Lay = LdsFull, bool kVerify = false, int kL = kNarrowLanes>
__device__ __forceinline__ void narrow_deferred(const PiecesArgs& a, const uint8_t* lds, uint64_t lo, uint64_t hi,
                                                uintptr_t dummy, VAcc& vacc) {
  constexpr uint32_t kPerGroup = 64 / kL;
  // The lane constants are recomputed here (volatile, so not merged with the kernel's own): values kept live across
  // the main group loop for this rarely taken walk would cost registers at the 16-wave kernels' 128-VGPR cap.
  uint32_t lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  const uint32_t lc0 = Lay::lc0(lane), lc1 = Lay::lc1(lane);
  const uint32_t j = lane & (kL - 1);
  const uint32_t slot = lane / kL;
  const uint32_t hint32 = uint32_t(a.hint);
  struct Desc {
    uint64_t off;
    uint32_t len, lenhi, init;
  };
  auto load_desc = [&](uint64_t g, Desc& d) {
    const uint64_t b = g + slot;
    const uint64_t bb = b < hi ? b : hi - 1;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);
    d.len = l.x;
    d.lenhi = l.y;
    d.init = *(a.init ? a.init + bb : &a.tabs->z4[0][0]);
  };
  {
    for (uint64_t g = lo; g < hi; g += kPerGroup) {
      Desc d;
      load_desc(g, d);
      uint64_t over = __builtin_amdgcn_ballot_w64(g + slot < hi && (d.lenhi != 0 || d.len > hint32));
      while (over) {
        const uint32_t k = uint32_t(__builtin_ctzll(over)) / kL;  // slot of the next deferred block
        over &= ~(((1ull << kL) - 1) << (k * kL));
        const uint32_t src = k * kL;
        const uint64_t boff = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(d.off >> 32)), int(src)))) << 32) |
                              uint32_t(__builtin_amdgcn_readlane(int(uint32_t(d.off)), int(src)));
        const uint64_t L = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(d.lenhi), int(src)))) << 32) |
                           uint32_t(__builtin_amdgcn_readlane(int(d.len), int(src)));
        const uint32_t binit = uint32_t(__builtin_amdgcn_readlane(int(d.init), int(src)));
        // parts of q <= 1 GiB bytes (the slot geometry is 32-bit), 8 at a time, one per slot; part p's raw register
        // (from ~init for part 0, from 0 for the others) is carried to the block's end and the parts XORed
        uint64_t q = (L + kPerGroup - 1) / kPerGroup;
        if (q > (1ull << 30)) q = 1ull << 30;
        const uint64_t nparts = (L + q - 1) / q;
        const uintptr_t blk = reinterpret_cast<uintptr_t>(a.base) + boff;
        uint32_t acc = 0;
        for (uint64_t p0 = 0; p0 < nparts; p0 += kPerGroup) {
          const uint64_t p = p0 + slot;
          const uint64_t rs = p < nparts ? p * q : L;
          const uint64_t re = rs + q < L ? rs + q : L;
          NStaged<kG> X;
          nstage<kG, kNT, kAlignN, kL>(X, blk + rs, uint32_t(re - rs), j, dummy);
          uint32_t km = 0, kn = ~0u;
#pragma unroll
          for (uint32_t t = 0; t < kPerGroup; ++t) {
            const uint32_t kk = uint32_t(__builtin_amdgcn_readlane(int(X.K), int(t * kL)));
            km = km > kk ? km : kk;
            kn = kn < kk ? kn : kk;
          }
          uint32_t reg = nfinish<kG, kNT, kAlignN, Lay, kL>(lds, X, p == 0 ? ~binit : 0u, j, lc0, lc1, kn, km, dummy,
                                                         NoMid());
          if (j == kL - 1) reg = gf2_shift(a.tabs, reg, L - re);  // carried to the block's end
#pragma unroll
          for (uint32_t t = 0; t < kPerGroup; ++t)
            acc ^= uint32_t(__builtin_amdgcn_readlane(int(reg), int(t * kL + kL - 1)));
        }
        if (lane == 0) emit_block(a, g + k, ~acc);
        // acc is wave-uniform (a readlane sum); so is the stored word, read through readfirstlane
        if (kVerify) verify_uniform(vacc, g + k, ~acc, uint32_t(__builtin_amdgcn_readfirstlane(int(ld32(a.expect + g + k)))));
      }
    }
  }
}

// Unsplit batches only (every block <= 64 KiB <= piece_bytes); static contiguous runs of 8-block groups.
// Lay: the LDS layout (LdsFull: one workgroup per CU; LdsCompact: two).  The runs follow gridDim, so a grid of more
// workgroups than fit at once is the same computation (the hardware dispatcher then hands out the runs).
// kVerify: the verify form (verify_wave after each group; the stored words are loaded just before the next group's
// staging).
template <int kG, bool kNT, int kThreads, bool kOverlap = false, bool kAlignN = true, typename Lay = LdsFull,
          bool kVerify = false, typename Ext = Exact>
__global__ void __launch_bounds__(kThreads) crc32c_narrow_kernel(PiecesArgs a) {
  constexpr uint32_t kWavesPerWg = kThreads / 64;
  // LdsCompact is sized so that exactly two workgroups share a CU; the verify form's gather slots (verify_gather, 12 B
  // a wave) would push it past that and silently halve the occupancy (ADVICE r5)
  static_assert(!(kVerify && Lay::kCompact), "the verify form does not fit the compact two-workgroup LDS image");
  static_assert(!Lay::kCompact || 2 * Lay::kBytes <= 163840, "two compact images per CU");
  __shared__ __attribute__((aligned(16))) uint8_t lds[Lay::kBytes];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t j = lane & (kNarrowLanes - 1);
  const uint32_t slot = lane / kNarrowLanes;
  const uint32_t lc0 = Lay::lc0(lane);
  const uint32_t lc1 = Lay::lc1(lane);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t nwaves = uint64_t(gridDim.x) * kWavesPerWg;
  const uintptr_t dummy = reinterpret_cast<uintptr_t>(a.tabs);
  constexpr uint32_t kPerGroup = 64 / kNarrowLanes;

  // contiguous run of whole groups per wave.  Runs are numbered wave-major (run w*grid + b), so when there are
  // fewer groups than waves the busy waves are spread over every CU instead of filling the first CUs.
  const uint64_t groups = (a.count + kPerGroup - 1) / kPerGroup;
  const uint64_t gper = (groups + nwaves - 1) / nwaves;
  const uint64_t lo = (uint64_t(wave) * gridDim.x + blockIdx.x) * gper * kPerGroup;
  uint64_t hi = lo + gper * kPerGroup;
  if (hi > a.count) hi = a.count;

  // Descriptors run one group ahead of the staging: taking group g stages its rows from descriptors loaded
  // when group g-8 was taken, then loads those of group g+8 (each lane its slot's block: one 64-B line per
  // array, shared by the slot's 8 lanes), so no descriptor load sits between two groups' row loads.
  // The raw loaded words are kept and only used at the take, a group later: nothing consumes them right
  // after the loads, so the compiler's wait for them lands at the take, not behind the loads.
  // The kernel is chosen on the caller's max_len hint (<= 32 KiB), but a hint is never trusted for exactness: a
  // block longer than the hint (a.hint) is left out of its group and redone by its wave at the end of the run
  // (`deferred`), with its full 64-bit length.  The staged length stays 32-bit: a 64-bit block end spills at 16
  // waves.
  struct Desc {
    uint64_t off;
    uint32_t len, lenhi, init;
  };
  auto load_desc = [&](uint64_t g, Desc& d) {  // block g + slot; past hi: loads stay in bounds, take() empties it
    // slot through an empty asm: otherwise (g + 16 + slot) becomes a hoisted 64-bit lane constant that, at 128
    // VGPRs, is spilled and reloaded per group with a vmcnt(0) wait that drains the next group's row loads
    uint32_t sl = slot;
    asm volatile("" : "+v"(sl));
    const uint64_t b = g + sl;
    const uint64_t bb = b < hi ? b : hi - 1;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);  // one 8-B load, both words consumed at the take
    d.len = l.x;
    d.lenhi = l.y;
    d.init = *(a.init ? a.init + bb : &a.tabs->z4[0][0]);  // no init: a word that is 0 (Z_4 of byte 0)
  };
  struct NItem {  // the slot's block is g + slot (g: the group's first block, wave-uniform)
    uint32_t reg0;
    uint32_t kmin, kmax;
    bool over;  // this lane's block exceeds the hint: skipped here, redone at the end of the run
  };
  Desc dn;  // descriptors of the next group to take
  bool deferred = false;  // wave-uniform: some block of this wave's run exceeded the hint
  VAcc vacc;              // the verify form's verdict of this wave
  const uint32_t hint32 = uint32_t(a.hint);  // <= 64 KiB (route::decide)
  auto take = [&](uint64_t g, NItem& it, NStaged<kG>& st) {
    const bool in = g + slot < hi;
    const bool over = in && (dn.lenhi != 0 || dn.len > hint32);
    deferred |= __builtin_amdgcn_ballot_w64(over) != 0;
    const bool live = in && !over;
    const uintptr_t ps = live ? reinterpret_cast<uintptr_t>(a.base) + dn.off : dummy;
    it.reg0 = ~dn.init;
    it.over = over;
    nstage<kG, kNT, kAlignN>(st, ps, live ? dn.len : 0u, j, dummy);
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
  auto step = [&](uint64_t g, NItem& ia, NStaged<kG>& A, NItem& ib, NStaged<kG>& B) {
    const uint64_t gn = g + kPerGroup;
    // the next group is staged inside nfinish, after this group's last row loads; unconditional (past the
    // end it is an empty group of dummy loads: see the wide kernel's step())
    // the verify form: this group's stored words (uniform base + a clamped 32-bit lane offset), issued before the
    // group's remaining row loads and the next group's staging, so their latency hides under the group and the wait
    // for them is a counted vmcnt (see verify_wave)
    uint32_t ex = 0;
    if (kVerify) {
      const uint64_t last = hi - 1 - g;
      ex = ld32(a.expect + g + (slot < last ? slot : uint32_t(last)));
      __builtin_amdgcn_sched_barrier(0);
    }
    const uint32_t reg = nfinish<kG, kNT, kAlignN, Lay, kNarrowLanes, Ext>(lds, A, ia.reg0, j, lc0, lc1, ia.kmin,
                                                                         ia.kmax, dummy, [&]() { take(gn, ib, B); });
    const bool mine = j == kNarrowLanes - 1 && g + slot < hi && !ia.over;
    // compare before the store: a store between the stored word's load and its wait (in a branch the wait must also
    // cover when skipped) would make that wait one count short and hold up the next group's first staged load
    if (kVerify) verify_wave(vacc, mine, g, slot, ~reg, ex);
    if (mine) emit_block(a, g + slot, ~reg);
    load_desc(gn + kPerGroup, dn);  // here, where this group's registers are dead
    return gn < hi;
  };

  NItem cur, nxt;
  NStaged<kG> S, T;
  KVSEP_NSTAMP_ENTRY();  // stamp hooks (crc32c_hooks.inc): empty in the shipped library
  // The first group's descriptors are fetched during the LDS fill.  Staging its rows before the fill as well
  // measured 4-7 % slower on 256 MiB-1 GiB batches of 4 KiB blocks: the fill then waits behind them.
  if (kOverlap) {
    // descriptors, then the table loads, then the first group's rows: the LDS stores wait for the tables
    // only, so the first HBM round trip overlaps the fill.  Unconditional (an idle wave stages an empty
    // group), so the store's wait count is the same on every path.
    load_desc(lo, dn);
    auto mid = [&]() {
      take(lo, cur, S);
      load_desc(lo + kPerGroup, dn);
    };
    if constexpr (Lay::kCompact) fill_lds_compact<kThreads>(lds, &a.tabs->znarrow[0][0], a.tabs, tid, mid);
    else fill_lds<kThreads, true>(lds, &a.tabs->znarrow[0][0], a.tabs, tid, mid);
    __syncthreads();
  } else {
    if (lo < hi) load_desc(lo, dn);
    if constexpr (Lay::kCompact) fill_lds_compact<kThreads>(lds, &a.tabs->znarrow[0][0], a.tabs, tid);
    else fill_lds<kThreads, true>(lds, &a.tabs->znarrow[0][0], a.tabs, tid);
    __syncthreads();
    if (lo < hi) {
      take(lo, cur, S);
      load_desc(lo + kPerGroup, dn);
    }
  }
  KVSEP_NSTAMP(1);
  if (lo < hi) {
    for (uint64_t g = lo;; g += 2 * kPerGroup) {
      const bool more = step(g, cur, S, nxt, T);
      KVSEP_NSTEP();
      if (!more) break;
      const bool more2 = step(g + kPerGroup, nxt, T, cur, S);
      KVSEP_NSTEP();
      if (!more2) break;
    }
  }
  KVSEP_NSTAMP(7);
  if (deferred) narrow_deferred<kG, kNT, kAlignN, Lay, kVerify>(a, lds, lo, hi, dummy, vacc);
  if (kVerify) verify_publish<kWavesPerWg>(a, wave, vacc);
}

// Batches of short blocks up to ~1 GiB (route::Form::Claim, form 10, round 4): the workgroup owns a contiguous run of 8-block
// groups and deals it to its 8 waves through an LDS claim counter (one ds_add per group: lgkmcnt, never in the rows'
// vmcnt stream), so the waves the memory system serves first take more of the run.  Otherwise the narrow kernel's
// pipeline: a group's rows are staged inside the previous group's finish, and the group after that is claimed and its
// descriptors loaded right after the previous group's emit.  Measured against the shipped forms in one process
// (tools/narrow_variants_probe.py, 4 KiB blocks, graph replay; profiles/round4/queue_variants/): 128 MiB 26.1 vs 28.2
// us, 256 MiB (config 2) 45.3 vs 48.4, 512 MiB 82.5 vs 90.5, 1 GiB 154.6 vs 165.3 -- but 2 GiB 346.8 vs 313.8 and 4 GiB
// 641.8 vs 622.1 (the wave-major runs of the 8-wave narrow kernel stream better there).  The same run dealt round-robin
// with no claims measured within 1 % of the claims: most of the gain is the workgroup-contiguous run itself.  Blocks
// over the hint go to narrow_deferred right after their group (8 waves have the VGPRs for it inline).
// kVerify: the verify form (stored words loaded before each group's remaining rows, verify_wave, verify_publish).
// kOverlap (shipped): the first group's rows are staged between the fill's table loads and its LDS stores, so the
// first HBM round trip runs under the fill (diag variant 59 = without: 4 KiB blocks 128 MiB 25.60 -> 24.84 us, 256 MiB
// 44.75 -> 44.15, 512 MiB 81.83 -> 81.29, 1 GiB 156.09 -> 154.77; profiles/round4/claim_shapes/).
// kL: lanes per slot -- 16 makes a group 4 blocks (Z_256 rows, the tree tables' Z_256 replicated; narrow form 11, see
// route::decide's claim16 rule; diag variant 60 is the same kernel).
// kLean (round 6, VERDICT r5's config-2 levers): bit 0 the fill fetches each table entry once (fill_lds<kOnce>), bit 1
// the head / tail loads only for groups that have a head or tail chunk (nstage<kSkipHT>), bit 2 no initial-register
// load when the batch has no inits (a launch-uniform branch).
template <int kG, int kThreads, bool kVerify = false, bool kOverlap = true, int kL = kNarrowLanes, uint32_t kLean = 0>
__global__ void __launch_bounds__(kThreads) crc32c_narrow_claim_kernel(PiecesArgs a) {
  constexpr uint32_t kWaves = kThreads / 64, kPerGroup = 64 / kL, kNone = 0xffffffffu;
  [[maybe_unused]] constexpr uint32_t kWavesPerWg = kWaves;  // the stamp hooks' name for it
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  __shared__ uint32_t claimed;  // groups of the run claimed after each wave's first (static) one
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t j = lane & (kL - 1);
  const uint32_t slot = lane / kL;
  const uint32_t lc0 = LdsFull::lc0(lane), lc1 = LdsFull::lc1(lane);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uintptr_t dummy = reinterpret_cast<uintptr_t>(a.tabs);
  const uint64_t count = a.count;
  const uint32_t hint32 = uint32_t(a.hint);  // <= 64 KiB (route::decide)
  // this workgroup's contiguous run of groups [run0, run1); group indices fit 32 bits (count < 2^32)
  const uint32_t groups = uint32_t((count + kPerGroup - 1) / kPerGroup);
  const uint32_t per_wg = (groups + gridDim.x - 1) / gridDim.x;
  const uint32_t run0 = blockIdx.x * per_wg < groups ? blockIdx.x * per_wg : groups;
  const uint32_t run1 = run0 + per_wg < groups ? run0 + per_wg : groups;
  if (tid == 0) claimed = 0;  // before the fill's barrier; every claim comes after it

  bool ended = false;
  auto next_group = [&]() -> uint32_t {  // claims only after the barrier; none once the run is used up
    if (ended) return kNone;
    uint32_t c = 0;
    if (lane == 0) c = atomicAdd(&claimed, 1u);
    c = uint32_t(__builtin_amdgcn_readfirstlane(int(c)));
    const uint32_t g = run0 + kWaves + c;
    ended = g >= run1;
    return ended ? kNone : g;
  };
  struct Desc {
    uint64_t off;
    uint32_t len, lenhi, init;
  };
  auto load_desc = [&](uint32_t g, Desc& d) {  // past the batch: loads stay in bounds, take() empties the slot
    uint32_t sl = slot;
    asm volatile("" : "+v"(sl));  // see load_desc in crc32c_narrow_kernel
    const uint64_t blk = uint64_t(g) * kPerGroup + sl;
    const bool in = g != kNone && blk < count;
    const uint64_t bb = in ? blk : 0;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);
    d.len = l.x;
    d.lenhi = l.y;
    if (kLean & 4u) d.init = a.init ? *(a.init + bb) : 0u;  // (bb = 0 past the batch: in bounds)
    else d.init = *(a.init && in ? a.init + bb : &a.tabs->z4[0][0]);  // no init: a word that is 0 (Z_4 of byte 0)
  };
  struct CItem {
    uint32_t g, reg0, kmin, kmax;
    bool over, deferred;
  };
  Desc dn;
  auto take = [&](uint32_t g, CItem& it, NStaged<kG>& st) {
    const uint64_t blk = uint64_t(g) * kPerGroup + slot;
    const bool in = g != kNone && blk < count;
    const bool over = in && (dn.lenhi != 0 || dn.len > hint32);
    it.deferred = __builtin_amdgcn_ballot_w64(over) != 0;
    const bool live = in && !over;
    it.g = g;
    it.over = over;
    it.reg0 = ~dn.init;
    nstage<kG, true, true, kL, (kLean & 2u) != 0>(st, live ? reinterpret_cast<uintptr_t>(a.base) + dn.off : dummy,
                                                  live ? dn.len : 0u, j, dummy);
    uint32_t km = 0, kn = ~0u;
#pragma unroll
    for (uint32_t k = 0; k < kPerGroup; ++k) {
      const uint32_t kk = uint32_t(__builtin_amdgcn_readlane(int(st.K), int(k * kL)));
      km = km > kk ? km : kk;
      kn = kn < kk ? kn : kk;
    }
    it.kmax = km;
    it.kmin = kn;
  };
  uint32_t gn = kNone;  // the group staged next (its descriptors are in dn until its take)
  VAcc vacc;            // the verify form's verdict of this wave
  auto step = [&](CItem& ia, NStaged<kG>& A, CItem& ib, NStaged<kG>& B) -> bool {
    const uint64_t g0 = uint64_t(ia.g) * kPerGroup;
    uint32_t ex = 0;
    if (kVerify) {  // this group's stored words, before its remaining rows (see crc32c_narrow_kernel's step)
      const uint64_t last = count - 1 - g0;
      ex = ld32(a.expect + g0 + (slot < last ? slot : uint32_t(last)));
      __builtin_amdgcn_sched_barrier(0);
    }
    const uint32_t reg = nfinish<kG, true, true, LdsFull, kL>(lds, A, ia.reg0, j, lc0, lc1, ia.kmin, ia.kmax, dummy,
                                                    [&]() { take(gn, ib, B); });
    const bool mine = j == kL - 1 && g0 + slot < count && !ia.over;
    if (kVerify) verify_wave(vacc, mine, g0, slot, ~reg, ex);  // before the store
    if (mine) emit_block(a, g0 + slot, ~reg);
    if (ia.deferred)  // wave-uniform: this group's blocks over the hint, whole
      narrow_deferred<kG, true, true, LdsFull, kVerify, kL>(a, lds, g0, g0 + kPerGroup < count ? g0 + kPerGroup : count,
                                                        dummy, vacc);
    gn = next_group();  // the group after ib: claimed now, its descriptors loaded while ib runs
    load_desc(gn, dn);
    return ib.g != kNone;
  };

  // the wave's first group is static (the wave's slot of the run), its descriptors fetched during the LDS fill
  KVSEP_NSTAMP_ENTRY();  // stamp hooks (crc32c_hooks.inc): empty in the shipped library
  uint32_t g0 = run0 + wave < run1 ? run0 + wave : kNone;
  load_desc(g0, dn);
  CItem cur, nxt;
  NStaged<kG> S, T;
  const uint32_t* rep = kL == 8 ? &a.tabs->znarrow[0][0] : &a.tabs->ztree[4][0][0];  // Z_{16 kL}
  if (kOverlap) {  // unconditional: a wave with no group stages an empty one (the stores' wait count is fixed)
    fill_lds<kThreads, kL == 8, (kLean & 1u) != 0>(lds, rep, a.tabs, tid, [&]() { take(g0, cur, S); });
    __syncthreads();
  } else {
    fill_lds<kThreads, kL == 8, (kLean & 1u) != 0>(lds, rep, a.tabs, tid);
    __syncthreads();
  }
  KVSEP_NSTAMP(1);
  if (g0 != kNone) {
    if (!kOverlap) take(g0, cur, S);
    gn = next_group();
    load_desc(gn, dn);
    for (;;) {  // (stamps: after each group but a wave's last)
      if (!step(cur, S, nxt, T)) break;
      KVSEP_NSTEP();
      if (!step(nxt, T, cur, S)) break;
      KVSEP_NSTEP();
    }
  }
  KVSEP_NSTAMP(7);
  // two-level arrival: the claims balance the run, so the 256 workgroups end within a µs of each other (bunched, as
  // the combine kernel's do), unlike the other narrow forms' staircase of workgroup ends
  if (kVerify) verify_publish<kWaves, kVaccShards>(a, wave, vacc);
}

// Bitonic sort of one (key, idx) pair per lane over the wavefront, ascending by key (ties by idx, so the two
// lanes of every compare-exchange agree): 21 ds_bpermute stages of two values each.
__device__ __forceinline__ void wave_sort64(uint32_t& key, uint32_t& idx, uint32_t lane) {
  asm volatile("" : "+v"(lane));  // opaque: keeps the 21 stages' lane ^ j addresses from being hoisted as constants
#pragma unroll
  for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
      const int addr = int((lane ^ jj) << 2);
      const uint32_t pk = uint32_t(__builtin_amdgcn_ds_bpermute(addr, int(key)));
      const uint32_t pi = uint32_t(__builtin_amdgcn_ds_bpermute(addr, int(idx)));
      const bool up = (lane & k) == 0;  // this lane's bitonic block sorts ascending
      const bool low = (lane & jj) == 0;
      const bool pless = pk < key || (pk == key && pi < idx);
      const bool take = (low == up) ? pless : !pless;  // the low lane of an ascending pair keeps the minimum
      key = take ? pk : key;
      idx = take ? pi : idx;
    }
  }
}

// Ragged batches of short blocks (see route::decide): the narrow kernel's 8-block groups, but formed from 64-block
// windows sorted by length, so a group's 8 blocks are of similar length and its slots do not wait for one long
// block.  Lane i holds the descriptor of block W + i of window W (loaded a window ahead); after the sort, group k's
// slot s takes the block at sorted position 8k + s (two ds_bpermutes to find it, four to fetch its descriptor).
// The rows, the slot tree and the end path are the narrow kernel's (nstage / nfinish); blocks over the hint go to
// narrow_deferred as there.
// Ext::sorted_emit / sorted_join / kDrain: empty in Exact; the KVSEP_DIAG build's types put the round-3 bisection's
// compare variants there (crc32c_diag.inc; the bisection tools were retired in round 6, commit 8853f41).
template <int kG, bool kNT, int kThreads, bool kVerify = false, typename Ext = Exact>
__global__ void __launch_bounds__(kThreads) crc32c_narrow_sorted_kernel(PiecesArgs a) {
  constexpr uint32_t kWavesPerWg = kThreads / 64;
  constexpr uint32_t kPerGroup = 64 / kNarrowLanes;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t j = lane & (kNarrowLanes - 1);
  const uint32_t slot = lane / kNarrowLanes;
  const uint32_t lc0 = (lane & 31u) << 2;
  const uint32_t lc1 = lc0 | 0x10000u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t nwaves = uint64_t(gridDim.x) * kWavesPerWg;
  const uintptr_t dummy = reinterpret_cast<uintptr_t>(a.tabs);
  const uint64_t groups = (a.count + kPerGroup - 1) / kPerGroup;
  const uint64_t gper = (groups + nwaves - 1) / nwaves;
  const uint64_t lo = (uint64_t(wave) * gridDim.x + blockIdx.x) * gper * kPerGroup;  // wave-major runs
  uint64_t hi = lo + gper * kPerGroup;
  if (hi > a.count) hi = a.count;
  const uint32_t hint32 = uint32_t(a.hint);  // <= 64 KiB (route::decide)
  // window descriptor of block W + lane; len: the length, kOver (longer than the hint: deferred) or kPast (past hi)
  constexpr uint32_t kOver = 0xffffffffu, kPast = 0xfffffffeu;
  struct WDesc {  // (the initial register is loaded per group, a group ahead of its use: two VGPRs less)
    uint64_t off;
    uint32_t len, idx;  // idx: after the sort, the window lane holding sorted position `lane`
  };
  auto load_win = [&](uint64_t W, WDesc& d) {
    const uint64_t b = W + lane;
    const bool in = b < hi;
    const uint64_t bb = in ? b : hi - 1;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);
    d.len = !in ? kPast : (l.y != 0 || l.x > hint32) ? kOver : l.x;
  };
  auto sort_win = [&](WDesc& d) {
    uint32_t key = d.len == kOver ? 0u : d.len;  // deferred blocks are empty in this pass: they sort first
    d.idx = lane;
    wave_sort64(key, d.idx, lane);
  };
  struct NItem {
    uint64_t w;    // window base (wave-uniform)
    uint32_t src;  // this lane's slot's block: w + src
    uint32_t reg0, kmin, kmax;
    bool live;
  };
  bool deferred = false;
  VAcc vacc;  // the verify form's verdict of this wave
  auto take = [&](uint64_t W, const WDesc& d, uint32_t k, NItem& it, NStaged<kG>& st) {
    uint32_t sl = slot;
    asm volatile("" : "+v"(sl));  // see load_desc in crc32c_narrow_kernel
    const uint32_t src = uint32_t(__builtin_amdgcn_ds_bpermute(int((k * kPerGroup + sl) << 2), int(d.idx)));
    const int sa = int(src << 2);
    const uint32_t len = uint32_t(__builtin_amdgcn_ds_bpermute(sa, int(d.len)));
    const uint32_t offl = uint32_t(__builtin_amdgcn_ds_bpermute(sa, int(uint32_t(d.off))));
    const uint32_t offh = uint32_t(__builtin_amdgcn_ds_bpermute(sa, int(uint32_t(d.off >> 32))));
    deferred |= __builtin_amdgcn_ballot_w64(len == kOver) != 0;
    it.live = len < kPast;
    it.w = W;
    it.src = src;
    it.reg0 = ~*(a.init && it.live ? a.init + (W + src) : &a.tabs->z4[0][0]);  // z4[0][0] == 0
    const uintptr_t ps = it.live ? reinterpret_cast<uintptr_t>(a.base) + ((uint64_t(offh) << 32) | offl) : dummy;
    nstage<kG, kNT, true>(st, ps, it.live ? len : 0u, j, dummy);
    uint32_t km = 0, kn = ~0u;
#pragma unroll
    for (uint32_t t = 0; t < kPerGroup; ++t) {
      const uint32_t kk = uint32_t(__builtin_amdgcn_readlane(int(st.K), int(t * kNarrowLanes)));
      km = km > kk ? km : kk;
      kn = kn < kk ? kn : kk;
    }
    it.kmax = km;
    it.kmin = kn;
  };

  auto take_empty = [&](NItem& it, NStaged<kG>& st) {  // past the last group: the same loads, all to `dummy`
    it.live = false;
    it.w = 0;
    it.src = 0;
    it.reg0 = 0;
    uintptr_t d = dummy;
    asm volatile("" : "+s"(d));  // opaque: its loop-invariant addresses would otherwise be hoisted (and spilled)
    nstage<kG, kNT, true>(st, d, 0u, j, dummy);
    it.kmax = it.kmin = 0;
  };

  WDesc cw, nw;
  if (lo < hi) load_win(lo, cw);  // its round trip overlaps the LDS fill
  fill_lds<kThreads, true>(lds, &a.tabs->znarrow[0][0], a.tabs, tid);
  __syncthreads();
  if (lo < hi) {
    uint64_t W = lo, Wn = lo + 64;
    if (Wn < hi) load_win(Wn, nw);
    sort_win(cw);
    auto groups_in = [&](uint64_t w) { return uint32_t(((hi - w < 64 ? hi - w : 64) + kPerGroup - 1) / kPerGroup); };
    uint32_t k = 0, nk = groups_in(W);
    NItem cur, nxt;
    NStaged<kG> S, T;
    take(W, cw, 0, cur, S);
    // finish group k of window W (staged in ia / A) while the next group -- k + 1 of W, or the first group of the
    // next window, sorted right there -- is staged into ib / B
    auto step = [&](NItem& ia, NStaged<kG>& A, NItem& ib, NStaged<kG>& B) -> bool {
      const bool here = k + 1 < nk;
      const bool next_win = !here && Wn < hi;
      // the verify form: this group's stored words, issued before the group's remaining row loads and the next group's
      // staging, from one place on every path (so the wait for them is a counted vmcnt, never a drain; see verify_wave)
      uint32_t ex = 0;
      if (kVerify) {
        ex = ld32(a.expect + ia.w + (ia.live ? ia.src : 0u));
        __builtin_amdgcn_sched_barrier(0);
      }
      const uint32_t reg = nfinish<kG, kNT, true>(lds, A, ia.reg0, j, lc0, lc1, ia.kmin, ia.kmax, dummy, [&]() {
        if (here) {
          take(W, cw, k + 1, ib, B);
        } else if (next_win) {
          sort_win(nw);
          take(Wn, nw, 0, ib, B);
        } else {
          take_empty(ib, B);
        }
      });
      if (kVerify) verify_wave(vacc, j == kNarrowLanes - 1 && ia.live, ia.w, ia.src, ~reg, ex);  // before the store
      if (j == kNarrowLanes - 1 && ia.live) {
        emit_block(a, ia.w + ia.src, ~reg);
        Ext::sorted_emit(a, ia.w + ia.src, reg);
      }
      Ext::sorted_join(a, j == kNarrowLanes - 1 && ia.live, ia.w, ia.src, reg, lane);
      if (Ext::kDrain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (here) {
        ++k;
        return true;
      }
      if (!next_win) return false;
      cw = nw;
      W = Wn;
      Wn += 64;
      k = 0;
      nk = groups_in(W);
      if (Wn < hi) load_win(Wn, nw);
      return true;
    };
    for (;;) {
      if (!step(cur, S, nxt, T)) break;
      if (!step(nxt, T, cur, S)) break;
    }
  }
  if (deferred) narrow_deferred<kG, kNT, true, LdsFull, kVerify>(a, lds, lo, hi, dummy, vacc);
  if (kVerify) verify_publish<kWavesPerWg>(a, wave, vacc);
}

// ------------------------------------------------------------------------------------------------
// crc32c_narrow_coop_kernel (narrow form 12, round 6): batches of uniform short blocks (<= 4 KiB: config 2) with the
// workgroup's 8 waves on the SAME 8-block group.  Every narrow form before it gave each wave its own groups, so a
// workgroup's loads in flight sat in eight 32 KiB groups spread over 256 KiB; a read-only probe of that shape takes
// 39.5 us for 256 MiB, and the same slot rows with the workgroup's waves inside one 32 KiB window 36.4-36.8 us -- the
// streaming kernel's rate (tools/group_pattern_probe.hip modes 8 / 9, profiles/round6/).  Here:
//  * Slot s of every wave is block 8g + s; wave w takes the block's rows w, w + 8, w + 16, w + 24 (K <= 32 rows of
//    128 B for a block <= 4 KiB on the 128-B grid, as nstage cuts it), so each lane runs 4 stride chains 1 KiB apart
//    through the wide kernel's replicated Z_1024 (the workgroup holds the wide kernel's full LDS image), then the
//    STEP4W merge and the 3-level slot tree (Z_16, Z_32, Z_64): lane 8s + 7 holds the pending word at the end of the
//    wave's last row of block s.
//  * Those 8 words per block -- at the ends of rows K-8 .. K-1, wave (q + K) mod 8 at position q -- go through LDS
//    (one barrier per group, a buffer per staging role) to the block's combining wave, wave s, whose slot-s lanes
//    merge them with a second 3-level tree (Z_128, Z_256, Z_512) into the register at the rows' end, then add the
//    block's whole 16-B chunks after the rows and its tail bytes (nfinish's end path) and emit / verify it.  Each wave
//    combines one block per group.
//  * The head register (bytes before the first 16-B boundary, from ~init) enters wave 0's row-0 chain as the pending
//    word at h0 (nfinish's injection); a block with no rows gets it in its combining wave.
//  * Blocks longer than the hint (clamped to kCoopMaxLen by route::decide; never trusted) are left out of the group and
//    checksummed by their combining wave with the wide kernel's machinery (stage / finish, 1 KiB rows), any length.
// The barrier is `s_waitcnt lgkmcnt(0); s_barrier` only -- never a vmcnt wait: the next groups' rows stay in flight.
// MEASURED, NOT ROUTED (set_kernel("coop") only).  Bit-exact everywhere (tools/coop_probe.py; the -m gpu suite's coop
// cases; tests/test_isa_emulation.py), but on one MI355X against the claim kernel, graph replay, 4 KiB blocks: 128 MiB
// 37.2 vs 24.4 us, 256 MiB 67.3 vs 44.1, 1 GiB 258.1 vs 153.3 (profiles/round6/coop/).  One group (32 KiB) staged ahead
// measured 65.2 us at 256 MiB, two 67.3: not the read depth.  A workgroup spends ~2 us per group, the critical path
// of a group -- 4-deep fold chains, the Z_4 merge, two 3-level trees and a barrier, all 8 waves in the same phase --
// where the claim kernel's waves run 32-row chains independently (8x fewer merges per byte, no barrier).  The
// faster read pattern does not pay for that.
// kInit: the batch has per-block initial CRCs.  Without them no init word is loaded at all: a load on one side of a
// launch-uniform branch left its register pending at the loop latch, where the register copy of the loop-carried
// descriptor waited for every load in flight (vmcnt(0)) once per two groups.
template <bool kVerify = false, bool kInit = false>
__global__ void __launch_bounds__(512) crc32c_narrow_coop_kernel(PiecesArgs a) {
  constexpr uint32_t kWaves = 8, kPerGroup = 8, kNone = 0xffffffffu;
  [[maybe_unused]] constexpr uint32_t kWavesPerWg = kWaves;
  constexpr uint32_t kRow = 128;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
  __shared__ uint32_t part[3][kPerGroup][kWaves];  // [staging role][block of the group][wave]
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t j = lane & 7u;
  const uint32_t slot = lane >> 3;
  const uint32_t lc0 = LdsFull::lc0(lane), lc1 = LdsFull::lc1(lane);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uintptr_t dummy = reinterpret_cast<uintptr_t>(a.tabs);
  uint32_t vz;  // 0, opaque to the uniformity analysis (the wide machinery's head / tail loads, see stage())
  asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
  const uint64_t count = a.count;
  const uint32_t hint32 = uint32_t(a.hint);
  const uint32_t groups = uint32_t((count + kPerGroup - 1) / kPerGroup);
  const uint32_t per_wg = (groups + gridDim.x - 1) / gridDim.x;
  const uint32_t run0 = blockIdx.x * per_wg < groups ? blockIdx.x * per_wg : groups;
  const uint32_t run1 = run0 + per_wg < groups ? run0 + per_wg : groups;
  const bool comb = slot == wave;  // this lane's slot is the block this wave combines

  struct Desc {
    uint64_t off;
    uint32_t len, lenhi, init;
  };
  auto load_desc = [&](uint32_t g, Desc& d) {  // past the run: loads stay in bounds, take() empties the slot
    uint32_t sl = slot;
    asm volatile("" : "+v"(sl));  // see load_desc in crc32c_narrow_kernel
    const uint64_t blk = uint64_t(g) * kPerGroup + sl;
    const bool in = g != kNone && blk < count;
    const uint64_t bb = in ? blk : 0;
    d.off = a.off[bb];
    const uint2 l = *reinterpret_cast<const uint2*>(a.len + bb);
    d.len = l.x;
    d.lenhi = l.y;
    d.init = kInit ? *(a.init + bb) : 0u;
  };
  struct CStaged {
    uint32_t g;          // the group (kNone: empty)
    uintptr_t ps;        // the slot's block start (dummy when empty or deferred)
    uint32_t len;        // its length on the slot path (0 when empty or deferred)
    uint32_t init;       // its initial CRC
    bool over;           // longer than the hint: left to the combining wave's wide path
    uint4 A[4];          // rows wave, wave + 8, wave + 16, wave + 24 of the slot's block (dummy where absent)
    uint4 hc, tc;        // head chunk (wave 0 and the combining lanes), tail chunks (the combining lanes)
  };
  // Three staging roles (X0, X1, X2: group i in X[i mod 3]) and three descriptor buffers (D[i mod 3] holds group i's):
  // the step of group i loads the descriptors of group i + 3, then stages group i + 2's rows, then folds group i, so
  // two groups' rows (64 KiB per workgroup) are in flight through every fold -- one group ahead left 32 KiB per CU in
  // flight and the kernel at 4.1 TB/s, the rate that depth sustains at the loaded latency (round 6 measurement)
  Desc D0, D1, D2;
  auto take = [&](uint32_t g, CStaged& st, const Desc& dn) {
    const uint64_t blk = uint64_t(g) * kPerGroup + slot;
    const bool in = g != kNone && blk < count;
    const bool over = in && (dn.lenhi != 0 || dn.len > hint32);
    const bool live = in && !over;
    st.g = g;
    st.over = over;
    st.init = in ? dn.init : 0u;
    st.ps = live ? reinterpret_cast<uintptr_t>(a.base) + dn.off : dummy;
    st.len = live ? dn.len : 0u;
    const NGeo geo = ngeo<true, 8>(st.ps, st.len);
    const uintptr_t line = st.ps - geo.P;
    const uint32_t K = (geo.ar - geo.h0 + kRow - 1) / kRow;
    const uintptr_t rows = line + intptr_t(int32_t(geo.ar - K * kRow + j * 16u));  // row 0's chunk of this lane
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      const uint32_t r = wave + 8u * u;
      st.A[u] = ld16<true>(r < K ? rows + uintptr_t(r) * kRow : dummy);
    }
    // head / tail chunks only where some lane needs them (a wave-uniform ballot, as nstage<kSkipHT>)
    const bool need_h = (wave == 0 || comb) && geo.P < geo.h0;
    const bool need_t = comb && (geo.a1 < geo.E || geo.a1 > geo.ar);
    if (__builtin_amdgcn_ballot_w64(need_h || need_t) != 0) {
      st.hc = ld16(need_h ? line + (geo.P & ~15u) : dummy);
      const uint32_t m = (geo.a1 - geo.ar) >> 4;
      st.tc = ld16(comb && (j == 7 ? geo.a1 < geo.E : j + m >= 7) ? line + (geo.a1 - (kRow - 16u) + j * 16u) : dummy);
    } else {
      st.hc = st.tc = make_uint4(0, 0, 0, 0);
    }
  };
  // the head register at h0: ~init stepped over the bytes before the first 16-B boundary
  auto head_reg = [&](const CStaged& st, const NGeo& geo) -> uint32_t {
    uint32_t reg = ~st.init;
    if (geo.P < geo.h0)
      reg = serial16(lds, reg, st.hc, int(geo.P & 15u), int(geo.h0 - (geo.P & ~15u)), LdsFull::kZ4, LdsFull::kByte);
    return reg;
  };
  VAcc vacc;
  auto next_of = [&](uint32_t g) -> uint32_t { return g != kNone && g + 1 < run1 ? g + 1 : kNone; };
  // one group: the rows of this wave, its pending words to LDS, the barrier, the combine of block `wave`
  auto step = [&](CStaged& s, uint32_t par, CStaged& nx, const Desc& dn, Desc& dl) {
    const uint64_t g0 = uint64_t(s.g) * kPerGroup;
    const bool in = s.g != kNone && g0 + slot < count;
    // the verify form: the block's stored word, before the staging (so its wait is a counted vmcnt)
    uint32_t ex = 0;
    if (kVerify) ex = ld32(a.expect + (in ? g0 + slot : 0));
    // group i + 3's descriptors, then group i + 2's rows (with the descriptors the previous step loaded: waited for
    // with those rows' predecessors only) go out before this group's rows -- staged two steps ago -- are waited for:
    // a counted vmcnt through the folds, the barrier and the combine
    const uint32_t g2 = next_of(next_of(s.g));
    load_desc(next_of(g2), dl);
    take(g2, nx, dn);
    __builtin_amdgcn_sched_barrier(0);
    if (s.g == kNone) return;  // workgroup-uniform: the run ended on an earlier role's step
    const NGeo geo = ngeo<true, 8>(s.ps, s.len);
    const uint32_t K = (geo.ar - geo.h0 + kRow - 1) / kRow;
    const int32_t rel0 = int32_t(geo.ar - K * kRow + j * 16u);  // row 0's chunk from the line
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (wave < K) {  // per lane (K is the slot's): this wave has rows of the block
      uint4 v = s.A[0];
      if (wave == 0) {
        if (rel0 < int32_t(geo.h0)) v = make_uint4(0, 0, 0, 0);         // front-masked: before the block
        if (rel0 == int32_t(geo.h0)) v.x ^= head_reg(s, geo);           // the head register as pending word at h0
      }
      c0 = v.x;
      c1 = v.y;
      c2 = v.z;
      c3 = v.w;
#pragma unroll
      for (uint32_t u = 1; u < 4; ++u)
        if (wave + 8u * u < K) {
          c0 = fold_step(lds, c0, s.A[u].x, lc0, lc1);
          c1 = fold_step(lds, c1, s.A[u].y, lc0, lc1);
          c2 = fold_step(lds, c2, s.A[u].z, lc0, lc1);
          c3 = fold_step(lds, c3, s.A[u].w, lc0, lc1);
        }
    }
    uint32_t p = zmap_x(lds, kZ4Off, c0, c1);
    p = zmap_x(lds, kZ4Off, p, c2);
    p = zmap_x(lds, kZ4Off, p, c3);
    {
      const uint32_t o = row_shr<1>(p);
      if ((j & 1u) == 1u) p = zmap_x(lds, kTreeOff, o, p);
    }
    {
      const uint32_t o = row_shr<2>(p);
      if ((j & 3u) == 3u) p = zmap_x(lds, kTreeOff + 4096u, o, p);
    }
    {
      const uint32_t o = row_shr<4>(p);
      if ((j & 7u) == 7u) p = zmap_x(lds, kTreeOff + 8192u, o, p);
    }
    if (j == 7u) part[par][slot][wave] = p;  // zero when the wave has no rows of the block
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // the combine of block `wave` in lanes 8 wave .. 8 wave + 7: wave (q + K) mod 8's word at position q
    uint32_t x = part[par][slot][(j + K) & 7u];
    {
      const uint32_t o = row_shr<1>(x);
      if ((j & 1u) == 1u) x = zmap_x(lds, kTreeOff + 3u * 4096u, o, x);
    }
    {
      const uint32_t o = row_shr<2>(x);
      if ((j & 3u) == 3u) x = zmap_x(lds, kTreeOff + 4u * 4096u, o, x);
    }
    {
      const uint32_t o = row_shr<4>(x);
      if ((j & 7u) == 7u) x = zmap_x(lds, kTreeOff + 5u * 4096u, o, x);
    }
    uint32_t reg = K ? zmap(lds, kZ4Off, x) : head_reg(s, geo);  // lane 7: the register at ar
    // the whole chunks [ar, a1) in lanes 7-m .. 6 of the tail load and the tail bytes (nfinish's end path)
    const uint32_t m = comb ? (geo.a1 - geo.ar) >> 4 : 0u;
    if (__builtin_amdgcn_ballot_w64(m != 0)) {
      const uint4 e = j < 7u && j + m >= 7u ? s.tc : make_uint4(0, 0, 0, 0);
      uint32_t q = zmap_x(lds, kZ4Off, e.x, e.y);
      q = zmap_x(lds, kZ4Off, q, e.z);
      q = zmap_x(lds, kZ4Off, q, e.w);
      q = row_shr<1>(q);
      {
        const uint32_t o = row_shr<1>(q);
        if ((j & 1u) == 1u) q = zmap_x(lds, kTreeOff, o, q);
      }
      {
        const uint32_t o = row_shr<2>(q);
        if ((j & 3u) == 3u) q = zmap_x(lds, kTreeOff + 4096u, o, q);
      }
      {
        const uint32_t o = row_shr<4>(q);
        if ((j & 7u) == 7u) q = zmap_x(lds, kTreeOff + 8192u, o, q);
      }
      if (m & 1u) reg = zmap(lds, kTreeOff, reg);
      if (m & 2u) reg = zmap(lds, kTreeOff + 4096u, reg);
      if (m & 4u) reg = zmap(lds, kTreeOff + 8192u, reg);
      reg ^= zmap(lds, kZ4Off, q);
    }
    const uint32_t tb = geo.E - geo.a1;  // tail bytes after a1
    if (comb && tb) reg = serial16(lds, reg, s.tc, 0, int(tb), kZ4Off, kByteOff);
    const bool mine = comb && j == 7u && in && !s.over;
    if (kVerify) verify_wave(vacc, mine, g0, slot, ~reg, ex);
    if (mine) emit_block(a, g0 + slot, ~reg);
    // the combining wave's block over the hint: the wide kernel's item machinery, the whole wave on it
    const uint64_t ovm = __builtin_amdgcn_ballot_w64(comb && j == 0 && s.over);
    if (ovm) {  // wave-uniform
      const uint64_t b = g0 + wave;
      const uintptr_t ps = reinterpret_cast<uintptr_t>(a.base) + a.off[b];
      const uintptr_t pe = ps + a.len[b];
      uint32_t r0 = ~(kInit ? a.init[b] : 0u);
      if (ps < pe && (ps & 15u) && r0) r0 = gf2_mulmod(a.tabs->xinv[ps & 15u], r0);  // padded head (stage<kPad>)
      Staged<4> w;
      stage<4, true, true, true>(w, ps, pe, lane, dummy, vz);
      const uint32_t rw = finish<4, true, true, true, Exact>(lds, w, r0, lane, lc0, lc1, NoMid());
      if (lane == 0) emit_block(a, b, ~rw);
      if (kVerify) verify_uniform(vacc, b, ~uint32_t(__builtin_amdgcn_readlane(int(rw), 0)), ld32(a.expect + b));
      // this rare path's own loads (a row loop) end here: without the drain its unknown count of loads would make
      // every wait after the join a vmcnt(0) on the common path too
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
  };

  const uint32_t g0 = run0 < run1 ? run0 : kNone;
  const uint32_t g1 = next_of(g0), g2 = next_of(g1);
  CStaged X0, X1, X2;
  // the first two groups' rows go out between the fill's table loads and its LDS stores (the claim kernel's overlap)
  load_desc(g0, D0);
  fill_lds<512, false, true>(lds, &a.tabs->z1024[0][0], a.tabs, tid, [&]() {
    load_desc(g1, D1);
    load_desc(g2, D2);
    take(g0, X0, D0);
    take(g1, X1, D1);
  });
  __syncthreads();
  if (g0 != kNone) {
    // One exit, at the latch, after three steps that always stage: the step of an empty group returns right after
    // its staging, so on every path into the loop header the descriptors its take reads have loads behind them.  (A
    // break between steps went through a flow block that the waitcnt pass also sees falling into the header, with
    // those descriptors the last loads on it: a vmcnt(0) on every group.)
    for (;;) {
      step(X0, 0u, X2, D2, D0);  // group i: stages i + 2 into X2, loads i + 3's descriptors into D0
      step(X1, 1u, X0, D0, D1);
      step(X2, 2u, X1, D1, D2);
      if (X0.g == kNone) break;  // group i + 3
    }
  }
  if (kVerify) verify_publish<kWaves, kVaccShards>(a, wave, vacc);
}
