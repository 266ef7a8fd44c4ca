// crc32c_logwalk.inc -- the log / MANIFEST reader on the device (included once, inside namespace kvsep, by
// crc32c_device.hip): the physical-record walk of kvsep_log_walk and the accept rule of kvsep_log_accept_gaps over an
// image that is on the device, so that walk, checksum and verdict run on one stream with no host step (DESIGN.md §3.8).
//
// The log format is cut into 32 KiB blocks and no physical record spans two (db/log_reader.cc:189-272), so a lane owns
// a block and walks its headers on its own; what crosses a block's end is a record index, one `pending` bit and the
// stop index (log_run.h).  Kernels ordered by the stream alone: no atomics, no look-back across workgroups, no
// workgroup waits for another, and every scratch word a replay reads was written by that replay.
//
//   the walk   log_count_kernel     cnt[b] = the physical records of block b (a dependent chain of header loads).
//              the offsets pass     (crc32c_offsets.inc, as it is) over cnt[]: base[b] = the records before block b,
//                                   *nrec = their total.
//              log_fill_kernel      block b once more: record base[b] + k goes to off / len / stored / type when it is
//                                   below cap; the lanes then zero the elements from min(*nrec, cap) to cap.
//   the accept log_block_kernel     block b's records are the run of off[] from a lower bound of its first possible
//                                   offset; the lane follows ok[] / type[] through them, then re-reads the image where
//                                   they end (one header, more only where cap cut the arrays) to tell a skip from a
//                                   trailer: first[b], the block's `pending` state, its stop candidate, its
//                                   bad-length bytes.
//              log_stop_kernel      one workgroup: the minimum of the stop candidates.
//              log_accept_kernel    block b again, now with `pending` from the block before and the stop: accept[] /
//                                   gap[] for its records, its mismatch bytes, its bad-length bytes when the reader
//                                   got that far; the lanes then zero accept / gap from min(*nrec, cap) to cap.
//              log_totals_kernel    one workgroup: the sums of the two byte counts.
//
// Every decision comes from log_run.h, which tests/cpp/log_run_test.cc runs lane by lane on the CPU.  Memory touched:
// the image is read bytewise, at header positions inside [0, n) only, and never written; off / len / type / ok are read
// at indices < min(*nrec, cap); the outputs are written for exactly cap elements.

struct LogWalkArgs {
  const uint8_t* img;
  uint64_t n, nblocks;
  uint64_t* off;  // the four outputs are nullable
  uint64_t* len;
  uint32_t* stored;
  uint8_t* type;
  uint64_t cap;
  const unsigned long long* nrec;  // the caller's word, written by the offsets pass before the fill
  unsigned long long* cnt;         // scratch: records per block
  unsigned long long* base;        // scratch: records before each block
};

struct LogAcceptArgs {
  const uint8_t* img;
  uint64_t n, nblocks;
  const uint64_t* off;
  const uint64_t* len;
  const uint8_t* type;
  const uint8_t* ok;
  const unsigned long long* nrec;
  uint64_t cap;
  uint8_t* accept;
  uint8_t* gap;           // nullable
  uint64_t* dropped;      // nullable
  uint64_t* bad_length;   // nullable
  unsigned long long* first;   // scratch per block: index of its first record in the arrays
  unsigned long long* state;   // ... what it leaves in `pending` (logrun::Pending)
  unsigned long long* cand;    // ... its stop candidate, kNone without one
  unsigned long long* drop;    // ... its mismatch bytes
  unsigned long long* badlen;  // ... its bad-length bytes
  unsigned long long* stop;    // scratch: the stop index
};

// What stands at p of a block that ends at `end`; l and t are the header's when there is one.
__device__ __forceinline__ logrun::Head log_head(const uint8_t* img, uint64_t p, uint64_t end, uint64_t& l,
                                                 uint8_t& t) {
  if (!logrun::has_header(p, end)) return logrun::kTrailer;
  l = logrun::header_len(img[p + 4], img[p + 5]);
  t = img[p + 6];
  return logrun::classify(p, end, l, t);
}

__device__ __forceinline__ uint64_t log_lane() { return uint64_t(blockIdx.x) * logrun::kThreads + threadIdx.x; }

__global__ void __launch_bounds__(logrun::kThreads)
log_count_kernel(const uint8_t* img, uint64_t n, uint64_t nblocks, unsigned long long* cnt) {
  const uint64_t blk = log_lane();
  if (blk >= nblocks) return;
  const uint64_t end = logrun::block_end(blk, n);
  uint64_t p = logrun::block_begin(blk), k = 0, l = 0;
  uint8_t t = 0;
  while (log_head(img, p, end, l, t) == logrun::kRecord) {
    ++k;
    p = logrun::next_header(p, l);
  }
  cnt[blk] = k;
}

__global__ void __launch_bounds__(logrun::kThreads) log_fill_kernel(LogWalkArgs a) {
  const uint64_t blk = log_lane();
  if (blk < a.nblocks) {
    const uint64_t end = logrun::block_end(blk, a.n);
    uint64_t p = logrun::block_begin(blk), i = ld_word64(a.base + blk), l = 0;
    uint8_t t = 0;
    while (i < a.cap && log_head(a.img, p, end, l, t) == logrun::kRecord) {
      if (a.off) a.off[i] = logrun::rec_off(p);
      if (a.len) a.len[i] = logrun::rec_len(l);
      if (a.stored) a.stored[i] = logrun::header_stored(a.img[p], a.img[p + 1], a.img[p + 2], a.img[p + 3]);
      if (a.type) a.type[i] = t;
      ++i;
      p = logrun::next_header(p, l);
    }
  }
  // the padding: len 0 is a block kvsep_log_verify_device never dereferences
  const uint64_t lanes = uint64_t(gridDim.x) * logrun::kThreads;
  for (uint64_t i = logrun::held(ld_word64(a.nrec), a.cap) + blk; i < a.cap; i += lanes) {
    if (a.off) a.off[i] = 0;
    if (a.len) a.len[i] = 0;
    if (a.stored) a.stored[i] = 0;
    if (a.type) a.type[i] = 0;
  }
}

__global__ void __launch_bounds__(logrun::kThreads) log_block_kernel(LogAcceptArgs a) {
  const uint64_t blk = log_lane();
  if (blk >= a.nblocks) return;
  const uint64_t held = logrun::held(ld_word64(a.nrec), a.cap);
  const uint64_t begin = logrun::block_begin(blk), end = logrun::block_end(blk, a.n);
  uint64_t lo = 0;
  for (uint64_t hi = held, want = logrun::first_in_block(begin); lo < hi;) {
    const uint64_t mid = logrun::probe(lo, hi);
    if (logrun::probe_right(a.off[mid], want)) lo = mid + 1;
    else hi = mid;
  }
  bool dead = false, any = false;
  uint64_t cand = logrun::kNone, p = begin;
  for (uint64_t i = lo; i < held; ++i) {
    const uint64_t o = a.off[i];
    if (!logrun::in_block(o, begin, end)) break;
    const uint8_t ok = a.ok[i];
    if (cand == logrun::kNone && logrun::stops(dead, ok, a.type[i])) cand = i;
    dead = logrun::dies(dead, ok);
    any = true;
    p = logrun::after_record(o, a.len[i], end);
  }
  // where the arrays' records of this block end: a skip, a trailer, or (the arrays cut by cap) more records
  uint64_t l = 0;
  uint8_t t = 0;
  logrun::Head tail;
  while ((tail = log_head(a.img, p, end, l, t)) == logrun::kRecord) p = logrun::next_header(p, l);
  a.first[blk] = lo;
  a.state[blk] = logrun::block_pending(any, dead, tail);
  a.cand[blk] = cand;
  a.badlen[blk] = logrun::bad_length_bytes(tail, dead, begin, end, p);
}

__global__ void __launch_bounds__(logrun::kThreads)
log_stop_kernel(const unsigned long long* cand, uint64_t nblocks, unsigned long long* stop) {
  __shared__ unsigned long long sh[logrun::kThreads];
  const uint32_t t = threadIdx.x;
  uint64_t m = logrun::kNone;
  for (uint64_t b = t; b < nblocks; b += logrun::kThreads) m = logrun::stop_min(m, cand[b]);
  sh[t] = m;
  __syncthreads();
  for (uint32_t d = logrun::kThreads / 2; d; d >>= 1) {
    if (t < d) sh[t] = logrun::stop_min(sh[t], sh[t + d]);
    __syncthreads();
  }
  if (t == 0) *stop = sh[0];
}

__global__ void __launch_bounds__(logrun::kThreads) log_accept_kernel(LogAcceptArgs a) {
  const uint64_t blk = log_lane();
  const uint64_t held = logrun::held(ld_word64(a.nrec), a.cap);
  if (blk < a.nblocks) {
    const uint64_t stop = ld_word64(a.stop);
    const uint64_t begin = logrun::block_begin(blk), end = logrun::block_end(blk, a.n);
    const uint64_t lo = ld_word64(a.first + blk);
    uint64_t i = lo, dropped = 0;
    if (i < held && logrun::in_block(a.off[i], begin, end)) {
      bool pending = false, dead = false;
      for (uint64_t b = blk; b > 0; --b)  // the block before decides, unless it held nothing at all
        if (logrun::resolve(logrun::Pending(ld_word64(a.state + b - 1)), &pending)) break;
      for (; i < held; ++i) {
        const uint64_t o = a.off[i];
        if (!logrun::in_block(o, begin, end)) break;
        const logrun::Verdict v = logrun::judge(i, stop, dead, pending, a.ok[i], a.type[i]);
        a.accept[i] = v.accept;
        if (a.gap) a.gap[i] = v.gap;
        if (v.mismatch) dropped += logrun::mismatch_bytes(logrun::header_of(o), end);
        if (i <= stop) pending = false;  // a record the reader read takes the carried value with it
        dead = v.dead;
      }
    }
    a.drop[blk] = dropped;
    if (!logrun::counts_bad_length(i, stop)) a.badlen[blk] = 0;
  }
  const uint64_t lanes = uint64_t(gridDim.x) * logrun::kThreads;
  for (uint64_t i = held + blk; i < a.cap; i += lanes) {
    a.accept[i] = 0;
    if (a.gap) a.gap[i] = 0;
  }
}

__global__ void __launch_bounds__(logrun::kThreads)
log_totals_kernel(const unsigned long long* drop, const unsigned long long* badlen, uint64_t nblocks,
                  uint64_t* dropped, uint64_t* bad_length) {
  __shared__ unsigned long long sd[logrun::kThreads], sb[logrun::kThreads];
  const uint32_t t = threadIdx.x;
  uint64_t d = 0, b = 0;
  for (uint64_t k = t; k < nblocks; k += logrun::kThreads) {
    d += drop[k];
    b += badlen[k];
  }
  sd[t] = d;
  sb[t] = b;
  __syncthreads();
  for (uint32_t s = logrun::kThreads / 2; s; s >>= 1) {
    if (t < s) {
      sd[t] += sd[t + s];
      sb[t] += sb[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (dropped) *dropped = sd[0];
    if (bad_length) *bad_length = sb[0];
  }
}
