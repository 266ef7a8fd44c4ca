// crc32c_sstindex.inc -- the SST table reader on the device (included once, inside namespace kvsep, by
// crc32c_device.hip): the footer, the walk of the index block and the slot layout of the table form over a table image
// that is on the device, so that footer, index, checksums and verdict list run on one stream with no host step
// (DESIGN.md §3.11).
//
// An index block ends in its restart array and an entry at a restart point shares nothing with the entry before it,
// so a lane owns a restart run and walks it on its own; what crosses a run's end is the entry index and the stop, the
// lowest run with an error (sst_run.h).  Kernels ordered by the stream alone: no atomics, no look-back across
// workgroups, no workgroup waits for another, and every scratch word a replay reads was written by that replay.
//
//   sst_footer_kernel        one wavefront, lane 0: handles[4] and the status word from the last 48 bytes.
//   sst_index_count_kernel   a lane per run of the `runs` the scratch holds: the block's tail, its own restart and the
//                            one after it, then its entries (a dependent chain of byte loads): cnt[r] = its good
//                            entries, err[r] = its error.  An error of the whole block is lane 0's.  The workgroup's
//                            lowest run with an error goes to wgstop[workgroup] (a reduction in LDS).
//   sst_index_stop_kernel    one workgroup: the lowest of those; *keep_before and the stop's code.
//   the offsets pass         (crc32c_offsets.inc, as it is) over cnt[] with that keep_before: base[r] = the entries
//                            before run r (written over err[], which the stop kernel has read), kSkip past the stop;
//                            *nblocks = their total.
//   sst_index_fill_kernel    run r once more: entry base[r] + k goes to off / len when it is below the room for data
//                            blocks; the lanes then write the elements from there to cap (the table form's two footer
//                            handles, zeros); lane 0 writes *status.
//   sst_table_prep_kernel    the table form's read check, per slot: length and stored word for the CRC kernels.
//
// Every decision comes from sst_run.h, which tests/cpp/sst_run_test.cc runs lane by lane on the CPU.  Memory touched:
// the image is read bytewise and never written: the last 48 bytes, bytes of [index_off, index_off + index_len), the
// index block's type byte, and the 4-byte stored word of each listed handle that lies inside the image; off / len are
// written for exactly cap elements.

// rd(p) = byte p of the image.
struct SstImage {
  const uint8_t* img;
  __device__ __forceinline__ uint8_t operator()(uint64_t p) const { return img[p]; }
};

struct SstIndexArgs {
  const uint8_t* img;
  uint64_t n;
  const uint64_t* handle;  // device: index_off, index_len
  uint64_t runs;           // lanes that own a run: what the scratch holds
  // the table form (null in the walk alone): the footer's four handles and the status word its kernel wrote, the index
  // block's checksum as computed and as stored
  const uint64_t* handles;
  const uint32_t* crc;
  const uint32_t* stored;
  uint64_t* off;
  uint64_t* len;
  uint64_t cap;
  unsigned long long* nblocks;  // the caller's word, written by the offsets pass before the fill
  uint32_t* status;
  unsigned long long* stop;     // scratch: [keep_before, the stop's error word]
  unsigned long long* cnt;      // scratch: entries per run
  unsigned long long* errbase;  // scratch: a run's error, then (from the offsets pass on) its base
  unsigned long long* wgstop;   // scratch: per workgroup of the count kernel, its lowest run with an error
};

__device__ __forceinline__ uint64_t sst_lane() { return uint64_t(blockIdx.x) * sst::kThreads + threadIdx.x; }

__global__ void __launch_bounds__(sst::kFooterThreads)
sst_footer_kernel(const uint8_t* img, uint64_t n, uint64_t* handles, uint32_t* status) {
  if (threadIdx.x != 0) return;
  SstImage rd{img};
  const sst::Footer f = sst::footer(rd, n);
  for (int k = 0; k < 4; ++k) handles[k] = f.h[k];
  *status = f.status;
}

// The minimum (sst::Rule::stop_pick) of the workgroup's candidates, in LDS; thread 0 holds the result.
__device__ __forceinline__ uint64_t sst_stop_reduce(unsigned long long* sh, uint64_t mine) {
  const uint32_t t = threadIdx.x;
  sh[t] = mine;
  __syncthreads();
  for (uint32_t d = sst::kThreads / 2; d; d >>= 1) {
    if (t < d) sh[t] = sst::Rule::stop_pick(sh[t], sh[t + d]);
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(sst::kThreads) sst_index_count_kernel(SstIndexArgs a) {
  __shared__ unsigned long long sh[sst::kThreads];
  const uint64_t r = sst_lane();
  uint64_t cand = sst::kNone;
  if (r < a.runs) {
    SstImage rd{a.img};
    const uint64_t ioff = a.handle[0], ilen = a.handle[1];
    uint32_t pre = sst::kOk;
    if (a.handles) {
      const uint32_t fs = *a.status;
      // the type byte lies inside the image when the footer passed (a usable handle)
      pre = sst::gate(fs, fs ? 0 : *a.crc, fs ? 0 : sst::unmask(*a.stored), fs ? uint8_t(0) : rd(ioff + ilen));
    }
    const sst::Counted c = sst::count_lane(rd, a.n, ioff, ilen, pre, a.runs, r);
    a.cnt[r] = c.cnt;
    a.errbase[r] = c.err;
    cand = sst::stop_candidate(r, c.err);
  }
  const uint64_t m = sst_stop_reduce(sh, cand);
  if (threadIdx.x == 0) a.wgstop[blockIdx.x] = m;
}

__global__ void __launch_bounds__(sst::kThreads)
sst_index_stop_kernel(const unsigned long long* wgstop, uint64_t nwg, const unsigned long long* err,
                      unsigned long long* stop) {
  __shared__ unsigned long long sh[sst::kThreads];
  uint64_t m = sst::kNone;
  for (uint64_t w = threadIdx.x; w < nwg; w += sst::kThreads) m = sst::Rule::stop_pick(m, wgstop[w]);
  const uint64_t s = sst_stop_reduce(sh, m);
  if (threadIdx.x == 0) {
    const uint64_t e = s == sst::kNone ? 0 : err[s];
    stop[0] = sst::keep_before(s, e);
    stop[1] = e;
  }
}

__global__ void __launch_bounds__(sst::kThreads) sst_index_fill_kernel(SstIndexArgs a) {
  const uint64_t g = sst_lane();
  const bool table = a.handles != nullptr;
  const uint64_t limit = sst::data_cap(table, a.cap);
  if (g < a.runs) {
    SstImage rd{a.img};
    sst::fill_lane(rd, a.handle[0], a.handle[1], g, ld_word64(a.errbase + g), limit,
                   [&](uint64_t k, uint64_t o, uint64_t l) {
                     const uint64_t i = ld_word64(a.errbase + g) + k;
                     if (i >= limit) return false;
                     a.off[i] = o;
                     a.len[i] = l;
                     return true;
                   });
  }
  const uint64_t nblocks = ld_word64(a.nblocks);
  const uint64_t m = sst::held(nblocks, limit);
  const uint64_t lanes = uint64_t(gridDim.x) * sst::kThreads;
  for (uint64_t i = m + g; i < a.cap; i += lanes) {
    a.off[i] = sst::after_data(table, i, m, a.handles, 0);
    a.len[i] = sst::after_data(table, i, m, a.handles, 1);
  }
  if (g == 0) *a.status = sst::final_status(sst::code_of(ld_word64(a.stop + 1)), table, nblocks, a.cap);
}

struct SstPrepArgs {
  const uint8_t* img;
  uint64_t n;
  const uint64_t* off;
  const uint64_t* len;
  uint64_t count;
  const unsigned long long* nblocks;  // null: the index block alone (count == 1), listed unless the footer is bad
  const uint32_t* status;
  uint64_t cap;
  uint64_t* len1;
  uint32_t* stored;
};

__global__ void __launch_bounds__(sst::kThreads) sst_table_prep_kernel(SstPrepArgs a) {
  const uint64_t i = sst_lane();
  if (i >= a.count) return;
  const uint32_t st = *a.status;
  const uint64_t real = a.nblocks ? sst::listed(st, ld_word64(a.nblocks), a.cap) : (st == sst::kBadFooter ? 0 : 1);
  const uint64_t o = a.off[i], l = a.len[i];
  const sst::Prep p = sst::prep(i < real, o, l, a.n);
  SstImage rd{a.img};
  uint32_t stored = p.read ? sst::le32(rd, o + l + 1) : p.stored;
  // every load has landed before the first store is issued (see offsets_tile_scan_kernel)
  asm volatile("" : "+v"(stored) : : "memory");
  a.len1[i] = p.len1;
  a.stored[i] = stored;
}
