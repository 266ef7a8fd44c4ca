// crc32c_vlogwalk.inc -- the value-log reader on the device (included once, inside namespace kvsep, by
// crc32c_device.hip): the header walk of kvsep_vlog_walk and the totals of kvsep_vlog_verify_host over an image that is
// on the device, so that walk, checksum and verdict run on one stream with no host step (DESIGN.md §3.13).
//
// vlog records lie back to back with no block structure (db/value_log_reader.cc:86-138), so the position of header
// i + 1 is known only from header i: the chain is serial in one 64-bit number.  One wavefront follows it.
//
//   the walk    vlog_walk_kernel    one workgroup of one wavefront.  The walk state (p, k, the window's bounds) is
//                                   wave-uniform and lives in scalar registers.  A refill stages a window of the image
//                                   in LDS with one batch of independent aligned 16-byte loads, every lane's loads
//                                   issued before the first wait; a step whose header lies in the window makes no
//                                   global load, it reads three LDS words.  Records are collected 64 at a time, one per
//                                   lane, and stored coalesced, masked by cap; the lanes then write the padding from
//                                   min(k, cap) to cap, and lane 0 the two result words.
//   the totals  vlog_totals_kernel  one wavefront: the verify call's first_bad / nbad, *nrec, cap and the arrays into
//                                   *ngood, *good_bytes, *drop_bytes (and the caller's first_bad / nbad words when the
//                                   verify call wrote the scratch's).
//
// Kernels ordered by the stream alone: no atomics, no memset node, no polling, no scratch; a replayed graph reads
// nothing the replay did not write.  Every decision comes from vlog_run.h, which tests/cpp/vlog_run_test.cc runs lane
// by lane on the CPU.  Memory touched: the image is read in naturally aligned 16-byte granules that each hold at least
// one byte of [base, base + n), and never written; with n == 0 base is not dereferenced; off / len / stored are written
// for exactly cap elements; the totals kernel reads off / len at g - 1 and g only.

struct VlogWalkArgs {
  const uint8_t* img;
  uint64_t n;
  uint64_t* off;  // the three arrays are nullable
  uint64_t* len;
  uint32_t* stored;
  uint64_t cap;
  unsigned long long* nrec;
  unsigned long long* consumed;  // nullable
};

struct VlogTotalsArgs {
  const unsigned long long* first_bad_in;  // the verify call's words; null: nothing was checked (cap == 0)
  const unsigned long long* nbad_in;
  const unsigned long long* nrec;
  const uint64_t* off;
  const uint64_t* len;
  uint64_t cap;
  unsigned long long* first_bad;  // the caller's words, each nullable, written when they are not the verify call's
  unsigned long long* nbad;
  unsigned long long* ngood;  // nullable
  unsigned long long* good_bytes;
  unsigned long long* drop_bytes;
};

// Element first + lane of the arrays for the lanes below cnt, masked by cap.
__device__ __forceinline__ void vlog_emit(const VlogWalkArgs& a, uint64_t first, uint32_t cnt, uint32_t lane,
                                          uint64_t o, uint64_t l, uint32_t st) {
  const uint64_t i = vlogrun::emit_index(first, lane);
  if (!vlogrun::emit_store(lane, cnt, i, a.cap)) return;
  if (a.off) a.off[i] = o;
  if (a.len) a.len[i] = l;
  if (a.stored) a.stored[i] = st;
}

__global__ void __launch_bounds__(vlogrun::kLanes) vlog_walk_kernel(VlogWalkArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t win[(vlogrun::kWindow + vlogrun::kLdsSlack) / 4];
  const uint32_t lane = threadIdx.x & (vlogrun::kLanes - 1);  // (the launch is one wavefront: every slot test folds)
  const uint64_t addr = reinterpret_cast<uintptr_t>(a.img), n = a.n;
  if (lane < vlogrun::kLdsSlack / 4) win[vlogrun::kWindow / 4 + lane] = 0;  // the header read's words past the window
  uint64_t p = 0, k = 0, lo = 0, hi = 0;  // wave-uniform; [lo, hi) = the staged bytes, none yet
  uint32_t sk = 0;
  uint64_t my_off = 0, my_len = 0;  // the record this lane holds of the batch being collected
  uint32_t my_stored = 0;
  while (vlogrun::has_header(p, n)) {
    if (!vlogrun::staged(p, lo, hi)) {  // refill at p
      sk = vlogrun::skew(addr, p);
      lo = p;
      hi = vlogrun::window_hi(p, sk, n);
      const uint32_t count = vlogrun::granule_count(p, sk, hi);
      uint4 v[vlogrun::kLoadsPerLane];
#pragma unroll
      for (uint32_t r = 0; r < vlogrun::kLoadsPerLane; ++r)
        v[r] = ld16(vlogrun::granule_addr(addr, p, sk, vlogrun::load_granule(vlogrun::load_slot(lane, r), count)));
      __syncthreads();  // (one wavefront: the steps before this refill have read the window)
#pragma unroll
      for (uint32_t r = 0; r < vlogrun::kLoadsPerLane; ++r) {
        const uint32_t slot = vlogrun::load_slot(lane, r);
        if (vlogrun::slot_in_lds(slot)) reinterpret_cast<uint4*>(win)[slot] = v[r];
      }
      __syncthreads();
    }
    const uint32_t idx = vlogrun::lds_index(p, lo, sk), w = vlogrun::lds_word(idx);
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(win[w]), w1 = __builtin_amdgcn_readfirstlane(win[w + 1]),
                   w2 = __builtin_amdgcn_readfirstlane(win[w + 2]);
    const uint64_t h = vlogrun::header_of_words(idx, w0, w1, w2), l = vlogrun::header_len(h);
    if (!vlogrun::has_payload(p, l, n)) break;
    if (lane == vlogrun::emit_lane(k)) {
      my_off = vlogrun::rec_off(p);
      my_len = l;
      my_stored = vlogrun::header_stored(h);
    }
    ++k;
    if (vlogrun::batch_full(k)) vlog_emit(a, vlogrun::batch_first(k, vlogrun::kLanes), vlogrun::kLanes, lane, my_off, my_len, my_stored);
    p = vlogrun::next_header(p, l);
  }
  const uint32_t tail = vlogrun::tail_count(k);
  vlog_emit(a, vlogrun::batch_first(k, tail), tail, lane, my_off, my_len, my_stored);
  // the padding: an empty block whose stored word is Mask(0) passes the verify call and is never dereferenced
  for (uint64_t i = vlogrun::pad_first(k, a.cap, lane); i < a.cap; i += vlogrun::kLanes) {
    if (a.off) a.off[i] = 0;
    if (a.len) a.len[i] = 0;
    if (a.stored) a.stored[i] = vlogrun::kPadStored;
  }
  if (lane == 0) {
    *a.nrec = k;
    if (a.consumed) *a.consumed = p;
  }
}

__global__ void __launch_bounds__(vlogrun::kLanes) vlog_totals_kernel(VlogTotalsArgs a) {
  if (threadIdx.x != 0) return;
  const uint64_t first_bad = a.first_bad_in ? ld_word64(a.first_bad_in) : ~0ull;
  const uint64_t nbad = a.nbad_in ? ld_word64(a.nbad_in) : 0;
  if (a.first_bad && a.first_bad != a.first_bad_in) *a.first_bad = first_bad;
  if (a.nbad && a.nbad != a.nbad_in) *a.nbad = nbad;
  const uint64_t nrec = ld_word64(a.nrec);
  const uint64_t g = vlogrun::good_count(first_bad, nrec, a.cap);
  if (a.ngood) *a.ngood = g;
  if (a.good_bytes) *a.good_bytes = vlogrun::has_good(g) ? a.off[g - 1] + a.len[g - 1] : 0;
  if (a.drop_bytes) *a.drop_bytes = vlogrun::has_drop(g, nrec, a.cap) ? a.len[g] : 0;
}
