// crc32c_logchain.inc -- the chains pass (included once, inside namespace kvsep, by crc32c_device.hip): which physical
// records of a log / MANIFEST image join into the logical records log::Reader::ReadRecord returns, computed on the
// device from the accept[] / gap[] bytes the device reader wrote, so that walk, checksum, verdict, assembly, layout and
// copy run on one stream with no host step (DESIGN.md §3.9).
//
//   first[j]  = the first physical record of chain j,  first[nchain .. cap] = count = min(*nrec, cap),
//   whole[j]  = 1 when chain j is a record the reader returns,
//   frag_off[i] / frag_len[i] = the payload of physical record i,
// which are the first / keep / seg_off / seg_len of the offsets, pack and gather forms as they are.
//
// Record i is an op on a one-bit state (chain_run.h); the state before it is an exclusive scan under "the rightmost op
// that is not kKeep wins".  Three kernels ordered by the stream alone, as the offsets pass (crc32c_offsets.inc): no
// cross-workgroup counters, no look-back, no workgroup waits for another, and every scratch word a replay reads was
// written by that replay.
//
//   chain_tile_kernel   one workgroup per tile of chain::kTile records, a lane owns a record per row: per row two
//                       ballots; for both incoming states the chain starts and whole ends are counted, rows chained in
//                       registers, the four waves' summaries joined by thread 0 into sum[tile].
//   chain_scan_kernel   one workgroup: each thread a contiguous run of tiles; the composed ops scanned in LDS give each
//                       run its incoming state, the counts picked by that state are scanned again: in[tile] = the
//                       tile's incoming state and chain base, grand[2] = the chains and the whole chains.
//   chain_write_kernel  one workgroup per tile of cap + 1 elements: the state before each record again (ballots within
//                       a row, rows chained in registers, waves through LDS); a chain's first record writes first[j],
//                       its last whole[j]; every lane writes its record's fragment or its element's padding;
//                       workgroup 0 writes *nchain and *nwhole.
//
// Every decision comes from chain_run.h, which tests/cpp/chain_run_test.cc runs lane by lane on the CPU.  All cross-lane
// work (the ballots) runs in full EXEC: the loads are predicated, the votes are not.  Memory touched: type / accept /
// gap / off / len at indices < count only (the successor's index is clamped inside count); first is written for exactly
// cap + 1 elements, whole / frag_off / frag_len for exactly cap.

struct ChainArgs {
  const uint8_t* type;
  const uint8_t* accept;
  const uint8_t* gap;   // null: all zero
  const uint64_t* off;  // off / len / frag_off / frag_len: all four or none
  const uint64_t* len;
  const unsigned long long* nrec;
  uint64_t cap;
  uint64_t ntiles;  // chain::tile_count(cap): the tiles that have a summary
  uint64_t* first;
  uint8_t* whole;
  uint64_t* frag_off;
  uint64_t* frag_len;
  uint64_t* nchain;
  uint64_t* nwhole;          // nullable
  unsigned long long* sum;   // scratch per tile: chain::pack_summary
  unsigned long long* in;    // scratch per tile: chain::pack_in
  unsigned long long* grand; // scratch: [chains, whole chains]
};

// One record's three bytes; i < count.
struct ChainRec {
  uint8_t type, accept, gap;
};
__device__ __forceinline__ ChainRec chain_load(const ChainArgs& a, uint64_t i) {
  return {a.type[i], a.accept[i], a.gap ? a.gap[i] : uint8_t(0)};
}

__global__ void __launch_bounds__(chain::kThreads) chain_tile_kernel(ChainArgs a) {
  __shared__ unsigned long long wsum[chain::kWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t count = chain::held(ld_word64(a.nrec), a.cap);
  chain::Summary s = chain::empty_summary();
#pragma unroll
  for (uint32_t row = 0; row < chain::kRows; ++row) {
    const uint64_t i = chain::block_index(blockIdx.x, w, row, lane);
    const bool own = i < count;
    ChainRec r{0, 0, 0};
    if (own) r = chain_load(a, i);
    const chain::Op op = own ? chain::op_of(r.type, r.accept, r.gap) : chain::kKeep;
    const uint64_t nonkeep = __builtin_amdgcn_ballot_w64(op != chain::kKeep);
    const uint64_t set = __builtin_amdgcn_ballot_w64(op == chain::kSet);
    chain::Summary rs;
    rs.op = chain::row_op(nonkeep, set);
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const bool joins = own && chain::continues(r.type, r.accept, r.gap, chain::state_before(h != 0, nonkeep, set, lane));
      rs.starts[h] = uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(own && !joins)));
      rs.wholes[h] =
          uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(own && chain::whole_end(r.type, r.accept, joins))));
    }
    s = chain::then(s, rs);
  }
  if (lane == 0) wsum[w] = chain::pack_summary(s);
  __syncthreads();
  if (threadIdx.x == 0) {
    chain::Summary t = chain::empty_summary();
    for (uint32_t v = 0; v < chain::kWaves; ++v) t = chain::then(t, chain::unpack_summary(wsum[v]));
    a.sum[blockIdx.x] = chain::pack_summary(t);
  }
}

__global__ void __launch_bounds__(chain::kScanThreads)
chain_scan_kernel(const unsigned long long* sum, unsigned long long* in, unsigned long long* grand, uint64_t ntiles) {
  __shared__ uint32_t sho[chain::kScanThreads];
  __shared__ unsigned long long shc[chain::kScanThreads], shw[chain::kScanThreads];
  const uint32_t t = threadIdx.x;
  const offsets::Run r = offsets::scan_range(t, offsets::scan_run(ntiles), ntiles);
  // the state before each thread's run: an inclusive scan of the runs' composed ops, applied to idle
  chain::Op op = chain::kKeep;
  for (uint64_t i = r.s; i < r.e; ++i) op = chain::compose(op, chain::unpack_summary(ld_word64(sum + i)).op);
  sho[t] = op;
  __syncthreads();
  for (uint32_t d = 1; d < chain::kScanThreads; d <<= 1) {
    const chain::Op left = t >= d ? chain::Op(sho[t - d]) : chain::kKeep;
    __syncthreads();
    sho[t] = chain::compose(left, chain::Op(sho[t]));
    __syncthreads();
  }
  const bool run_in = t ? chain::apply(false, chain::Op(sho[t - 1])) : false;
  // the counts each run adds under that state
  unsigned long long c = 0, wh = 0;
  bool st = run_in;
  for (uint64_t i = r.s; i < r.e; ++i) {
    const chain::Summary s = chain::unpack_summary(ld_word64(sum + i));
    c += s.starts[st ? 1 : 0];
    wh += s.wholes[st ? 1 : 0];
    st = chain::apply(st, s.op);
  }
  shc[t] = c;
  shw[t] = wh;
  __syncthreads();
  for (uint32_t d = 1; d < chain::kScanThreads; d <<= 1) {
    const unsigned long long v = t >= d ? shc[t - d] : 0, vw = t >= d ? shw[t - d] : 0;
    __syncthreads();
    shc[t] += v;
    shw[t] += vw;
    __syncthreads();
  }
  unsigned long long at = t ? shc[t - 1] : 0;
  const unsigned long long all = shc[chain::kScanThreads - 1], allw = shw[chain::kScanThreads - 1];
  st = run_in;
  for (uint64_t i = r.s; i < r.e; ++i) {
    unsigned long long word = ld_word64(sum + i);
    // the summary is in its register before the store is issued (see verdict_tile_scan_kernel)
    asm volatile("" : "+v"(word) : : "memory");
    const chain::Summary s = chain::unpack_summary(word);
    in[i] = chain::pack_in(st, at);
    at += s.starts[st ? 1 : 0];
    st = chain::apply(st, s.op);
  }
  if (t == 0) {
    grand[0] = all;
    grand[1] = allw;
  }
}

__global__ void __launch_bounds__(chain::kThreads) chain_write_kernel(ChainArgs a) {
  __shared__ uint32_t wop[chain::kWaves], wst[chain::kWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t count = chain::held(ld_word64(a.nrec), a.cap);
  const bool has = blockIdx.x < a.ntiles;  // the tile has a summary (uniform over the workgroup); else padding only
  uint64_t nchain = 0, nwhole = 0;
  if (a.ntiles) {
    nchain = ld_word64(a.grand);
    nwhole = ld_word64(a.grand + 1);
  }
  // every load comes before the first store: a record's bytes, its successor's, its walk entry
  ChainRec rec[chain::kRows] = {}, nx[chain::kRows] = {};
  uint64_t nonkeep[chain::kRows] = {}, set[chain::kRows] = {}, off[chain::kRows] = {}, len[chain::kRows] = {};
  bool own[chain::kRows] = {}, joins[chain::kRows] = {}, after[chain::kRows] = {};
  uint32_t rank[chain::kRows] = {};
  uint64_t before = 0;
  if (has) {
    const uint64_t tin = ld_word64(a.in + blockIdx.x);
    chain::Op mine = chain::kKeep;
#pragma unroll
    for (uint32_t row = 0; row < chain::kRows; ++row) {
      const uint64_t i = chain::block_index(blockIdx.x, w, row, lane);
      own[row] = i < count;
      if (own[row]) {
        rec[row] = chain_load(a, i);
        nx[row] = chain_load(a, chain::next_index(i, count));
        if (a.frag_off) {
          off[row] = a.off[i];
          len[row] = a.len[i];
        }
      }
      const chain::Op op = own[row] ? chain::op_of(rec[row].type, rec[row].accept, rec[row].gap) : chain::kKeep;
      nonkeep[row] = __builtin_amdgcn_ballot_w64(op != chain::kKeep);
      set[row] = __builtin_amdgcn_ballot_w64(op == chain::kSet);
      mine = chain::compose(mine, chain::row_op(nonkeep[row], set[row]));
    }
    if (lane == 0) wop[w] = mine;
    __syncthreads();
    // the state before this wave's first record: the tile's, then the waves before
    bool in = chain::in_state(tin);
    for (uint32_t u = 0; u < w; ++u) in = chain::apply(in, chain::Op(wop[u]));
    uint32_t starts = 0;
#pragma unroll
    for (uint32_t row = 0; row < chain::kRows; ++row) {
      const bool st = chain::state_before(in, nonkeep[row], set[row], lane);
      joins[row] = own[row] && chain::continues(rec[row].type, rec[row].accept, rec[row].gap, st);
      after[row] = chain::apply(st, own[row] ? chain::op_of(rec[row].type, rec[row].accept, rec[row].gap) : chain::kKeep);
      const uint64_t sb = __builtin_amdgcn_ballot_w64(own[row] && !joins[row]);
      // the starts of this wave up to and including this record
      rank[row] = starts + uint32_t(__builtin_popcountll(sb & chain::lanes_below(lane))) + (own[row] && !joins[row] ? 1u : 0u);
      starts += uint32_t(__builtin_popcountll(sb));
      in = chain::state_after_row(in, nonkeep[row], set[row]);
    }
    if (lane == 0) wst[w] = starts;
    __syncthreads();
    before = chain::in_base(tin);
    for (uint32_t u = 0; u < w; ++u) before += wst[u];
  }
#pragma unroll
  for (uint32_t row = 0; row < chain::kRows; ++row) {
    const uint64_t k = chain::block_index(blockIdx.x, w, row, lane);
    if (has && own[row]) {
      const uint64_t j = chain::chain_of(before, rank[row]);  // < nchain <= count <= cap
      if (!joins[row] && j <= a.cap) a.first[j] = k;
      if (chain::chain_ends(k, count, chain::continues(nx[row].type, nx[row].accept, nx[row].gap, after[row])) &&
          j < a.cap)
        a.whole[j] = chain::whole_end(rec[row].type, rec[row].accept, joins[row]) ? 1 : 0;
      if (a.frag_off) {
        a.frag_off[k] = chain::frag_off(off[row]);
        a.frag_len[k] = chain::frag_len(len[row]);
      }
    }
    if (a.first && chain::pads_first(k, nchain, a.cap)) a.first[k] = chain::pad_first(count);
    if (chain::pads_whole(k, nchain, a.cap)) a.whole[k] = 0;
    if (a.frag_off && chain::pads_frag(k, count, a.cap)) {
      a.frag_off[k] = 0;
      a.frag_len[k] = 0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *a.nchain = nchain;
    if (a.nwhole) *a.nwhole = nwhole;
  }
}

// rec_len[j] of the records composite: the offsets pass's extent of chain j (its record's bytes when whole, else 0).
__global__ void __launch_bounds__(chain::kThreads)
chain_reclen_kernel(const unsigned long long* ext, uint64_t* rec_len, uint64_t cap) {
  const uint64_t j = uint64_t(blockIdx.x) * chain::kThreads + threadIdx.x;
  if (j < cap) rec_len[j] = ld_word64(ext + j);
}
