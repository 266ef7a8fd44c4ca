// crc32c_logframe.inc -- the log / MANIFEST write side (included once, inside namespace kvsep, by crc32c_device.hip):
// records that lie in device memory become the bytes log::Writer::AddRecord (db/log_writer.cc:35-115) would append to a
// log of dest_length bytes, with no host step (DESIGN.md §3.10).
//
//   rec_at[i]     = where record i's first header goes, relative to the first appended byte; kSkip when dropped,
//   frag_first[i] = the fragments of the records before i,  frag_first[count] = *nfrag,
//   frag_off / frag_len / frag_at / frag_type [f] = fragment f's bytes, header position and type,
// which are the seg_off / seg_len / dst_off / types of the batched CRC and of the PackLog gather-copy as they are.
//
// Two kernels ordered by the stream alone, as the offsets and chains passes: no atomics, no look-back, no workgroup
// waits for another, no memset node, and every scratch word a replay reads was written by that replay.
//
//   logw_layout_kernel  one workgroup of one wavefront: the writer's block offset is a serial chain, taken 64 records
//                       a step.  A row's 7 + len are scanned in 32 bits (logw::reduce), the lanes whose record leaves
//                       a reset are balloted, the row is committed up to the first of them and the rest scanned again;
//                       with each lane's offset known, its fragment count and block advance are scanned as 64-bit
//                       values, rows chained in registers.  The len / keep of the next logw::kAhead rows are loaded
//                       before the current ones are resolved, so the chain waits for arithmetic, not for memory.
//                       Writes rec_at, frag_first, the per-record scratch word, *nfrag and *written.
//   logw_fill_kernel    a lane per fragment slot f < frag_cap: the owner search over frag_first (indices inside
//                       [0, count)), then the fragment's descriptors and CRC seed, or the slot's padding; a lane per
//                       record writes that record's pad zeros, byte by byte, inside [0, dst_bytes).
//
// Every decision comes from logw_run.h, which tests/cpp/logw_run_test.cc runs lane by lane on the CPU.  All cross-lane
// work (ballots, DPP, readlane) runs in full EXEC: the loads are predicated, the votes are not.  Memory touched: len and
// keep for count elements; off only for a laid record; rec_at and the scratch word for count, frag_first for
// count + 1; the fragment arrays and the seeds for exactly frag_cap.

struct LogwArgs {
  const uint64_t* off;
  const uint64_t* len;
  const uint8_t* keep;  // null: every record kept
  uint64_t count;
  uint32_t b0;  // logw::start_state(dest_length)
  uint8_t* dst;
  uint64_t dst_bytes;
  uint64_t* rec_at;
  uint64_t* frag_first;
  uint64_t* frag_off;
  uint64_t* frag_len;
  uint64_t* frag_at;
  uint8_t* frag_type;
  uint64_t frag_cap;
  uint64_t* nfrag;
  uint64_t* written;
  uint32_t* rec;    // scratch per record: logw::pack_rec
  uint32_t* seed;   // scratch per fragment slot: Value(&type, 1), the init of the fragment's checksum
  uint32_t s1, s2, s3, s4;  // Value(&type, 1) for FULL, FIRST, MIDDLE, LAST
};

template <int kStep>
__device__ __forceinline__ void logw_scan_step32(uint32_t& v, uint32_t lane) {
  constexpr uint32_t n = offsets::scan_shift(kStep);
  const uint32_t left = row_shr<int(n)>(v);  // every lane pulls: full EXEC, no branch
  v += offsets::scan_takes(lane, n) ? left : 0;
}

// The inclusive scan of v over the wavefront's 64 lanes (wave-uniform call sites only); the sums stay under 2^32.
__device__ __forceinline__ uint32_t logw_wave_scan32(uint32_t v, uint32_t lane) {
  logw_scan_step32<0>(v, lane);
  logw_scan_step32<1>(v, lane);
  logw_scan_step32<2>(v, lane);
  logw_scan_step32<3>(v, lane);
  const uint32_t t15 = uint32_t(__builtin_amdgcn_readlane(int(v), 15)), t31 = uint32_t(__builtin_amdgcn_readlane(int(v), 31)),
                 t47 = uint32_t(__builtin_amdgcn_readlane(int(v), 47));
  return v + uint32_t(offsets::row_base(lane, t15, t31, t47));
}

// The saturating inclusive scan of 64-bit values: in 32 bits when every lane's value is small enough that the row's
// sum cannot leave them (the common case: fragment counts and block advances of ordinary records), else the offsets
// pass's 64-bit scan.  The choice is wave-uniform by ballot.
__device__ __forceinline__ uint64_t logw_wave_scan64(uint64_t v, uint32_t lane) {
  if (__builtin_amdgcn_ballot_w64((v >> 26) != 0) == 0) return logw_wave_scan32(uint32_t(v), lane);
  return offsets_wave_scan(v, lane);
}

// len / keep of row `row` for this lane; a lane past the records holds a dropped record of length 0.
struct LogwRow {
  uint64_t len;
  uint8_t keep;
};
__device__ __forceinline__ LogwRow logw_load(const LogwArgs& a, uint64_t row, uint32_t lane) {
  const uint64_t i = row * logw::kWaveLanes + lane;
  LogwRow r{0, 0};
  if (i < a.count) {
    r.len = a.len[i];
    r.keep = a.keep ? a.keep[i] : uint8_t(1);
  }
  return r;
}

__global__ void __launch_bounds__(logw::kLayoutThreads) logw_layout_kernel(LogwArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t rows = logw::row_count(a.count);
  uint32_t r = a.b0;              // the raw offset in front of the row (wave-uniform)
  uint64_t block = 0, nfr = 0;    // blocks advanced and fragments so far (wave-uniform)
  LogwRow cur[logw::kAhead], nxt[logw::kAhead];
#pragma unroll
  for (uint32_t j = 0; j < logw::kAhead; ++j) cur[j] = logw_load(a, j, lane);
  for (uint64_t g = 0; g < rows; g += logw::kAhead) {
    // the next rows' loads do not depend on the state: issued before this group's chain
#pragma unroll
    for (uint32_t j = 0; j < logw::kAhead; ++j) nxt[j] = logw_load(a, g + logw::kAhead + j, lane);
#pragma unroll
    for (uint32_t j = 0; j < logw::kAhead; ++j) {
      if (g + j >= rows) break;  // wave-uniform
      const uint64_t i = (g + j) * logw::kWaveLanes + lane;
      const bool own = i < a.count, kept = own && cur[j].keep != 0;
      const uint64_t len = cur[j].len;
      const uint32_t x = logw::step_of(kept, len);
      const uint64_t km = __builtin_amdgcn_ballot_w64(kept);
      uint32_t rb = 0, ra = 0;  // the raw offset in front of this lane's record and behind it
      for (uint64_t todo = ~uint64_t(0); todo;) {  // wave-uniform: one turn, plus one per reset inside the row
        const bool mine = (todo >> lane) & 1;
        const uint32_t xs = mine ? x : 0;
        const uint32_t incl = logw_wave_scan32(xs, lane);
        const bool kb = (km & todo & logw::lanes_below(lane)) != 0;
        const uint32_t before = logw::raw_before(r, kb, incl - xs);
        const uint32_t behind = logw::raw_behind(r, kb || (mine && kept), incl);
        const uint64_t reset = __builtin_amdgcn_ballot_w64(mine && kept && logw::resets(behind));
        const uint64_t commit = logw::commit_mask(todo, reset);
        if ((commit >> lane) & 1) {
          rb = before;
          ra = behind;
        }
        r = uint32_t(__builtin_amdgcn_readlane(int(behind), int(logw::last_lane(commit))));
        todo &= ~commit;
      }
      const uint32_t b = logw::start_of(rb);
      const uint64_t nf = kept ? logw::nfrag(b, len) : 0;
      const uint64_t adv = kept ? logw::blocks_advanced(logw::resets(rb), nf) : 0;
      const uint64_t bend = logw::add_sat(block, logw_wave_scan64(adv, lane));
      const bool is_laid = logw::laid(kept, bend, ra);
      const uint64_t fr = logw::frags_of(is_laid, nf);
      const uint64_t fincl = logw_wave_scan64(fr, lane);  // a row's 64 counts cannot saturate: fincl - fr is exact
      if (own) {
        a.rec_at[i] = logw::rec_at(is_laid, bend, nf, b, a.b0);
        a.frag_first[i] = logw::add_sat(nfr, fincl - fr);
        a.rec[i] = logw::pack_rec(b, kept ? logw::pad_bytes(rb) : 0);
      }
      block = concat_readlane64(bend, 63);
      nfr = logw::add_sat(nfr, concat_readlane64(fincl, 63));
    }
#pragma unroll
    for (uint32_t j = 0; j < logw::kAhead; ++j) cur[j] = nxt[j];
  }
  if (lane == 0) {
    a.frag_first[a.count] = nfr;
    *a.nfrag = nfr;
    *a.written = logw::rel(logw::pos_sat(block, r), a.b0);
  }
}

__global__ void __launch_bounds__(logw::kFillThreads) logw_fill_kernel(LogwArgs a) {
  const uint64_t t = uint64_t(blockIdx.x) * logw::kFillThreads + threadIdx.x;
  const auto* ff = reinterpret_cast<const unsigned long long*>(a.frag_first);
  if (t < a.frag_cap) {
    const uint64_t nf = ld_word64(reinterpret_cast<const unsigned long long*>(a.nfrag));
    if (logw::pads_frag(t, nf, a.frag_cap)) {
      a.frag_off[t] = logw::kPadOff;
      a.frag_len[t] = logw::kPadLen;
      a.frag_at[t] = logw::kPadAt;
      a.frag_type[t] = logw::kPadType;
      a.seed[t] = logw::kPadSeed;
    } else {  // t < *nfrag = frag_first[count]: count != 0, and the owner is a laid record
      const uint64_t i = logw::owner(t, a.count, [&](uint64_t j) { return uint64_t(ld_word64(ff + j)); });
      const uint64_t k = t - ld_word64(ff + i);
      const uint32_t b = logw::rec_b(a.rec[i]);
      const uint64_t len = a.len[i];
      const uint8_t type = logw::frag_type(k, logw::nfrag(b, len));
      a.frag_off[t] = a.off[i] + logw::frag_begin(b, k);
      a.frag_len[t] = logw::frag_len(b, len, k);
      a.frag_at[t] = logw::frag_at(a.rec_at[i], b, k);
      a.frag_type[t] = type;
      a.seed[t] = logw::seed_of(type, a.s1, a.s2, a.s3, a.s4);
    }
  }
  if (t < a.count) {
    const uint64_t at = a.rec_at[t];
    const uint32_t pad = logw::rec_pad(a.rec[t]);
    if (logw::writes_pad(at, pad, ld_word64(ff + t), a.frag_cap, a.dst_bytes))
      for (uint32_t j = 0; j < pad; ++j) pack_st8(reinterpret_cast<uintptr_t>(a.dst) + (at - pad) + j, 0);
  }
}
