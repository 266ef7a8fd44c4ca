// crc32c_sstbuild.inc -- the SST table writer on the device (included once, inside namespace kvsep, by
// crc32c_device.hip): the index walk that also says where the keys lie, the index block builder, the metaindex block
// and the footer, so that a salvaged table becomes a table again on the stream that verified it (DESIGN.md §3.12).
//
// Kernels ordered by the stream alone: no atomics, no look-back across workgroups, no workgroup waits for another, no
// memset node, and every scratch word a replay reads was written by that replay.
//
//   sst_keys_count_kernel  sst_index_count_kernel under the keys walk's rule (sst::count_lane_keys): an entry that
//                          shares key bytes with the one before it has no contiguous key and stops the walk.  The stop
//                          kernel and the offsets pass follow as in the plain walk, unchanged.
//   sst_keys_fill_kernel   sst_index_fill_kernel, and key_off / key_len next to off / len.
//   sstw_size_kernel       a lane per entry: its encoded size (0 when dropped) and its kept flag.
//   the offsets pass       (crc32c_offsets.inc, as it is) twice: over the sizes for each entry's byte position and the
//                          entries' total, over the flags for each kept entry's rank and the kept count.
//   sstw_fill_kernel       a lane per entry.  The kept entries are contiguous in the block, so a wavefront's 64
//                          entries are one byte range of it: each lane stages its header, its key (gathered bytewise
//                          from key_base + key_off[i]) and its handle in LDS at the range's destination phase, and
//                          the wave stores the range as crc32c_pack_kernel stores a span -- byte stores before the
//                          first and after the last 16-B boundary, naturally aligned 16-B stores between.  A range
//                          over sstw::kStageBytes is written entry by entry by the whole wave, the key as a pack span.
//                          Restarts are whole words of their lanes.  Nothing is read-modify-written.  Global lane 0
//                          posts the block's position and length for the checksum.
//   the batched CRC        (as it is) over that one block.
//   sstw_tail_kernel       one wavefront: the trailer, *out_len, *status; in the table form the metaindex block, the
//                          footer and *table_bytes.
//   sstw_keep_kernel       the rewrite's keep mask over the table verify's slots.
//
// Every decision comes from sstw_run.h (and sst_run.h), which tests/cpp/sstw_run_test.cc runs lane by lane on the CPU.
// The fill and tail kernels form the same sstw::plan from the same words before they write anything, so a refused
// block leaves the destination untouched.  Memory touched: key_off / key_len / blk_off / blk_len (and keep) are read
// for count elements; key bytes are read only for kept entries, bytewise inside [key_off[i], key_off[i] + key_len[i])
// when the wave stages, inside the naturally aligned 16-B granules that hold such a byte when it does not; dst is
// written only inside the block and its trailer (the table form: from *data_end to the end of the footer).

struct SstKeysArgs {
  SstIndexArgs w;
  uint64_t* key_off;
  uint64_t* key_len;
};

__global__ void __launch_bounds__(sst::kThreads) sst_keys_count_kernel(SstIndexArgs a) {
  __shared__ unsigned long long sh[sst::kThreads];
  const uint64_t r = sst_lane();
  uint64_t cand = sst::kNone;
  if (r < a.runs) {
    SstImage rd{a.img};
    const uint64_t ioff = a.handle[0], ilen = a.handle[1];
    uint32_t pre = sst::kOk;
    if (a.handles) {
      const uint32_t fs = *a.status;
      pre = sst::gate(fs, fs ? 0 : *a.crc, fs ? 0 : sst::unmask(*a.stored), fs ? uint8_t(0) : rd(ioff + ilen));
    }
    const sst::Counted c = sst::count_lane_keys(rd, a.n, ioff, ilen, pre, a.runs, r);
    a.cnt[r] = c.cnt;
    a.errbase[r] = c.err;
    cand = sst::stop_candidate(r, c.err);
  }
  const uint64_t m = sst_stop_reduce(sh, cand);
  if (threadIdx.x == 0) a.wgstop[blockIdx.x] = m;
}

__global__ void __launch_bounds__(sst::kThreads) sst_keys_fill_kernel(SstKeysArgs k) {
  const SstIndexArgs& a = k.w;
  const uint64_t g = sst_lane();
  const bool table = a.handles != nullptr;
  const uint64_t limit = sst::data_cap(table, a.cap);
  if (g < a.runs) {
    SstImage rd{a.img};
    const uint64_t ioff = a.handle[0];
    sst::fill_lane_keys(rd, ioff, a.handle[1], g, ld_word64(a.errbase + g), limit,
                        [&](uint64_t e, uint64_t o, uint64_t l, uint64_t kat, uint64_t klen) {
                          const uint64_t i = ld_word64(a.errbase + g) + e;
                          if (i >= limit) return false;
                          a.off[i] = o;
                          a.len[i] = l;
                          k.key_off[i] = ioff + kat;
                          k.key_len[i] = klen;
                          return true;
                        });
  }
  const uint64_t nblocks = ld_word64(a.nblocks);
  const uint64_t m = sst::held(nblocks, limit);
  const uint64_t lanes = uint64_t(gridDim.x) * sst::kThreads;
  for (uint64_t i = m + g; i < a.cap; i += lanes) {
    a.off[i] = sst::after_data(table, i, m, a.handles, 0);
    a.len[i] = sst::after_data(table, i, m, a.handles, 1);
    k.key_off[i] = 0;
    k.key_len[i] = 0;
  }
  if (g == 0) *a.status = sst::final_status(sst::code_of(ld_word64(a.stop + 1)), table, nblocks, a.cap);
}

struct SstBuildArgs {
  const uint8_t* key_base;
  const uint64_t* key_off;
  const uint64_t* key_len;
  const uint64_t* blk_off;
  const uint64_t* blk_len;
  const uint8_t* keep;  // null: every entry with a laid-out block
  uint64_t count;
  uint8_t* dst;
  uint64_t dst_bytes;
  const unsigned long long* at;  // device: where the block goes (the table form: *data_end)
  uint64_t lead, trail;          // the table form: the metaindex block before, the footer after
  const uint32_t* source;        // the rewrite: the walk's status word (null: none)
  unsigned long long* size;      // scratch, per entry
  unsigned long long* flag;
  unsigned long long* pos;
  unsigned long long* rank;
  unsigned long long* words;     // scratch: sstw::Word
  uint64_t* out_len;
  uint32_t* status;
  uint64_t* table_bytes;         // the table form only
  uint32_t meta_masked;          // ... the empty block's trailer word
  const DevTables* tabs;
};

__device__ __forceinline__ uint64_t sstw_lane() { return uint64_t(blockIdx.x) * sstw::kThreads + threadIdx.x; }

__device__ __forceinline__ sstw::Plan sstw_plan(const SstBuildArgs& a) {
  return sstw::plan(ld_word64(a.words + sstw::kEntriesBytes), ld_word64(a.words + sstw::kNKept), ld_word64(a.at),
                    a.lead, a.trail, a.dst_bytes, a.source ? *a.source : 0u);
}

__global__ void __launch_bounds__(sstw::kThreads) sstw_size_kernel(SstBuildArgs a) {
  const uint64_t i = sstw_lane();
  if (i >= a.count) return;
  const uint64_t bo = a.blk_off[i];
  const bool keep = sstw::kept(a.keep ? a.keep[i] : uint8_t(1), bo);
  a.size[i] = sstw::entry_size(keep, a.key_len[i], bo, a.blk_len[i]);
  a.flag[i] = keep ? 1 : 0;
}

__global__ void __launch_bounds__(sstw::kThreads) sstw_fill_kernel(SstBuildArgs a) {
  __shared__ uint4 stage[sstw::kWaves][sstw::kStageGranules];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t i = sstw_lane();
  const uint64_t entries = ld_word64(a.words + sstw::kEntriesBytes), nkept = ld_word64(a.words + sstw::kNKept);
  const sstw::Plan p = sstw_plan(a);
  if (i == 0) {
    a.words[sstw::kCrcOff] = p.at;
    a.words[sstw::kCrcLen] = p.len;
  }
  const bool go = p.status == sstw::kOk;  // uniform over the grid
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(a.dst) + p.at;
  const uintptr_t kb = reinterpret_cast<uintptr_t>(a.key_base);
  bool mine = false;
  uint64_t pos = 0, sz = 0, rk = 0, kl = 0, ko = 0, ho = 0, hl = 0;
  if (go && i < a.count && ld_word64(a.flag + i)) {
    mine = true;
    pos = ld_word64(a.pos + i), sz = ld_word64(a.size + i), rk = ld_word64(a.rank + i);
    kl = a.key_len[i], ko = a.key_off[i], ho = a.blk_off[i], hl = a.blk_len[i];
  }
  // the wave's kept entries are the bytes [w0, w1) of the block (wave-uniform)
  const uint64_t kept = __builtin_amdgcn_ballot_w64(mine);
  uint64_t w0 = 0, n = 0;
  if (kept) {
    w0 = concat_readlane64(pos, __builtin_ctzll(kept));
    n = concat_readlane64(pos + sz, 63 - __builtin_clzll(kept)) - w0;
  }
  const bool staged = kept && sstw::stages(n);
  const uint32_t phase = uint32_t((d0 + w0) & (sstw::kGran - 1));
  uint8_t* st = reinterpret_cast<uint8_t*>(&stage[wv][0]) + phase;
  if (staged && mine) {
    uint8_t* e = st + (pos - w0);
    const uint32_t h = sstw::head_len(kl), vl = sstw::value_len(ho, hl);
    for (uint32_t j = 0; j < h; ++j) e[j] = sstw::head_byte(j, kl, vl);
    for (uint64_t j = 0; j < kl; ++j) e[h + j] = pack_ld8(kb + ko + j);
    for (uint32_t j = 0; j < vl; ++j) e[h + kl + j] = sstw::value_byte(j, ho, hl);
  }
  __syncthreads();
  if (staged) {
    const uintptr_t d = d0 + w0;
    const sstw::Span s = sstw::split(d, n);
    if (lane < s.head + s.tail) {
      const uint64_t e = sstw::edge_index(s, n, lane);
      pack_st8(d + e, st[e]);
    }
    const uint32_t g0 = uint32_t((phase + s.head) / sstw::kGran);  // a whole granule of the stage when there is a body
    for (uint64_t g = lane; g < s.body; g += sstw::kWaveLanes) {
      const uint4 v = stage[wv][g0 + g];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      pack_st16(d + s.head + g * sstw::kGran, w);
    }
  } else {
    // a range over the staging area: an entry at a time on all 64 lanes
    for (uint64_t todo = kept; todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint64_t epos = concat_readlane64(pos, src), ekl = concat_readlane64(kl, src);
      const uint64_t eko = concat_readlane64(ko, src), eho = concat_readlane64(ho, src), ehl = concat_readlane64(hl, src);
      const uint32_t h = sstw::head_len(ekl), vl = sstw::value_len(eho, ehl);
      if (lane < h + vl) {
        const uint64_t j = lane < h ? lane : lane + ekl;
        pack_st8(d0 + epos + j, sstw::frame_byte(j, ekl, eho, ehl));
      }
      if (ekl) pack_span(kb + eko, d0 + epos + h, ekl, lane);
    }
  }
  // the restart array: a word per kept entry, the count, and the empty block's one restart
  if (mine) {
    const uintptr_t r = d0 + sstw::restart_at(entries, rk, i);
    const uint32_t word = uint32_t(pos);
    for (uint32_t j = 0; j < 4; ++j) pack_st8(r + j, uint8_t(word >> (8 * j)));
  }
  if (go && i == 0) {
    const uintptr_t c = d0 + sstw::count_at(entries, nkept);
    const uint32_t word = sstw::count_word(nkept);
    for (uint32_t j = 0; j < 4; ++j) pack_st8(c + j, uint8_t(word >> (8 * j)));
    if (sstw::lone_restart(nkept))
      for (uint32_t j = 0; j < 4; ++j) pack_st8(d0 + entries + j, 0);
  }
}

__global__ void __launch_bounds__(sstw::kTailThreads) sstw_tail_kernel(SstBuildArgs a) {
  const uint32_t lane = threadIdx.x;
  const sstw::Plan p = sstw_plan(a);
  const uint64_t at0 = ld_word64(a.at);
  uint32_t l = ~*reinterpret_cast<const uint32_t*>(a.words + sstw::kCrc);
  l = a.tabs->byte1[l & 0xffu] ^ (l >> 8);  // Extend by the type byte 0: one STEP1 (util/crc32c.cc:287-292)
  const uint32_t masked = mask_crc(~l);
  if (lane == 0) {
    *a.out_len = p.need;
    *a.status = p.status;
    if (a.table_bytes) *a.table_bytes = sstw::table_bytes(p);
  }
  if (p.status != sstw::kOk) return;
  const uintptr_t d = reinterpret_cast<uintptr_t>(a.dst);
  const uintptr_t t = d + p.at + p.len;
  if (lane < sstw::kTrailer) pack_st8(t + lane, sstw::trailer_byte(lane, masked));
  if (!a.table_bytes) return;
  if (lane < sstw::kMetaFramed) pack_st8(d + at0 + lane, sstw::meta_byte(lane, a.meta_masked));
  if (lane < sstw::kFooter)
    pack_st8(t + sstw::kTrailer + lane, sstw::footer_byte(lane, at0, sstw::kEmptyBlock, p.at, p.len));
}

// The rewrite's keep mask over the table verify's cap slots: the data slots that passed, nothing after a source status
// that refuses the rewrite.
__global__ void __launch_bounds__(sstw::kThreads)
sstw_keep_kernel(const uint8_t* ok, const unsigned long long* nblocks, const uint32_t* status, uint64_t cap,
                 uint8_t* keep) {
  const uint64_t i = sstw_lane();
  if (i >= cap) return;
  keep[i] = !sstw::refuses(*status) && i < sst::held(ld_word64(nblocks), cap - 2) && ok[i] ? 1 : 0;
}
