// crc32c_device.hip -- CDNA4 (gfx950) kernels and the device-side C ABI of libkvsep_crc32c.
//
// Computes leveldb::crc32c::Extend (util/crc32c.cc:276-377) for batches of independent byte
// blocks resident in HBM.  Design:
//
//  * Work item = "piece": a block, or an end-aligned slice of at most `piece_bytes` of a long block
//    (pieces 1..k-1 are exactly piece_bytes long, piece 0 takes the remainder on top of a full piece, and the init CRC).
//  * One wavefront per piece.  The piece is cut at 16-byte-aligned addresses into
//      head  [ps, h0)   < 16 B, serial (word/byte steps),
//      body  [h0, a1)   16-B aligned, as rows of 1 KiB ending exactly at a1,
//      tail  [a1, pe)   < 16 B, serial.
//    In the body every lane loads one 16-B vector per row (global_load_dwordx4, one 1 KiB
//    coalesced wave-instruction per row) and owns four 32-bit "stride chains" -- the reference's
//    4-stride swath (util/crc32c.cc:332-348) widened to 256 strides, 1 KiB apart:
//        c' = word ^ Z_1024(c)
//    Z_1024 is evaluated as 4 byte-table lookups in LDS.  The four tables are replicated 32x so that
//    lane L always reads bank L%32: ds_read_b32 is conflict-free whatever the data.  The lookup
//    address (table pair, byte value, lane copy) is assembled by ONE v_perm_b32 per lookup.
//  * Chains are merged per lane with Z_4 (the STEP4W re-injection, util/crc32c.cc:307-315, 361-366),
//    then across the 64 lanes by a 6-level butterfly with Z_16 .. Z_512 (DPP/bpermute shuffles).
//  * Pieces of one block are merged by a tiny combine kernel: R(A||B) = Z_|B|(R(A)) ^ R(B).
//
// Every map Z_d ("advance the CRC register over d zero bytes") is generated on the host from the
// Castagnoli polynomial (gf2.h); no table is copied from the reference.
//
// One translation unit, in parts: crc32c_fold.inc (the shared device code), crc32c_wide.inc (the wide kernel),
// crc32c_narrow.inc (the narrow kernels for short blocks), crc32c_support.inc (combine, plan, helpers),
// crc32c_verdicts.inc (the list pass of the verify forms), crc32c_concat.inc (the batched combine), crc32c_pack.inc
// (the gather-copy of the pack and frame forms), crc32c_offsets.inc (the offsets pass of the salvage forms),
// crc32c_logwalk.inc (the log / MANIFEST walk and accept rule), crc32c_logchain.inc (the chains pass that joins FIRST /
// MIDDLE / LAST fragments), then this file's host side -- the context, kernel routing, launches and the device C ABI.  crc32c_hooks.inc holds the
// measurement hook points (empty in the shipped library), crc32c_diag.inc the KVSEP_DIAG build's A/B forms.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kvsep_crc32c.h"
#include "gf2.h"
#include "kvsep_testing.h"
#include "kvsep_internal.h"
#include "plan_size.h"
#include "route.h"
#include "concat_run.h"
#include "pack_run.h"
#include "offsets_run.h"
#include "log_run.h"
#include "chain_run.h"
#include "logw_run.h"
#include "sst_run.h"
#include "sstw_run.h"
#include "vlog_run.h"

namespace kvsep {

#include "crc32c_fold.inc"     // shared device code: tables, arguments, fold, staging, verify, LDS fill
#include "crc32c_wide.inc"     // crc32c_pieces_kernel
#include "crc32c_narrow.inc"   // crc32c_narrow_kernel, _claim_kernel, _sorted_kernel
#include "crc32c_support.inc"  // combine, plan, SST helpers, generator, streaming read
#include "crc32c_verdicts.inc" // the list pass of the verify forms: bad-block index list, per-block verdict bytes
#include "crc32c_concat.inc"   // crc32c_concat_kernel: the batched combine of the concat and gather forms
#include "crc32c_pack.inc"     // crc32c_pack_kernel: the byte-exact gather-copy of the pack and frame forms
#include "crc32c_offsets.inc"  // offsets_*_kernel: the masked offset scan of the offsets and salvage forms
#include "crc32c_logwalk.inc"  // log_*_kernel: the log / MANIFEST walk and accept rule, a lane per 32 KiB block
#include "crc32c_logchain.inc" // chain_*_kernel: the chains pass, FIRST / MIDDLE / LAST fragments into records
#include "crc32c_logframe.inc" // logw_*_kernel: the log / MANIFEST write side, records into fragments and pads
#include "crc32c_sstindex.inc" // sst_*_kernel: the SST footer, the index-block walk, the table form's slots
#include "crc32c_sstbuild.inc" // sst_keys_*_kernel, sstw_*_kernel: the walk with keys, the index block builder, the footer
#include "crc32c_vlogwalk.inc" // vlog_*_kernel: the vlog header walk through an LDS window, the read form's totals

}  // namespace kvsep

// ================================================================================================
// host side
using namespace kvsep;

// A graph capture's own scratch (round 6).  Every call captured into one graph -- one capture
// sequence, hipStreamGetCaptureInfo's id -- runs on the same capture set, and no other capture shares it while it is
// held, so two graphs replayed at once never share a plan, a work counter, SST arrays or verdict slots, and replays of
// one graph write identical words.  Sets are sized by kvsep_crc32c_reserve before capture (nothing is allocated under
// capture) and stay held, frozen in size, until kvsep_crc32c_release_captures: a graph keeps the pointers it captured.
struct CaptureSet {
  unsigned long long id = 0;
  bool held = false;
  Scratch sc;
};
constexpr size_t kDefaultCaptureSets = 4;

struct kvsep_crc32c_ctx {
  int device = 0;
  int num_cus = 0;
  DevTables* d_tabs = nullptr;
  uint64_t piece_bytes = 128 * 1024;  // best of 32 KiB .. 1 MiB on configs 3a/3b/4
  bool piece_auto = true;             // smaller pieces for small batches (piece_for); off once set explicitly
  int dynamic = -1;  // -1 auto, 0 static, 1 guided
  int kernel = 0;    // kvsep_crc32c_ctx_set_kernel, 0..8 (route::Kernel): 0 auto, 1 wide only, 2-8 narrow when the hint allows
  // what a routing decision reads (route.h)
  route::Settings settings() const { return {num_cus, piece_bytes, piece_auto, dynamic, route::Kernel(kernel)}; }
  uint32_t static_contig = 1;  // static schedule: contiguous runs (1) or round-robin items (0, set_schedule(2))
  Scratch sc;  // scratch of the calls made directly on this context (any stream, event-ordered)
  std::vector<std::unique_ptr<CaptureSet>> caps;  // scratch of captured calls, one set per graph capture
  uint64_t res_count = 0, res_bytes = 0;          // the largest reservation: what capture sets are sized for
  int host_node = -1;        // NUMA node of the device's PCI function (-1: unknown / not bound): host legs go there
  bool inject_failure = false;  // kvsep_crc32c_ctx_inject_failure: the next call fails right after its CRC kernel
  // timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
  std::vector<hipEvent_t> ev_pool;
  // host form
  HostStaging staging;
  std::mutex mu;
};

// The KVSEP_DIAG tools build's kernel variants, their per-context selection and host hooks; in the shipped library the
// hooks are constant-false inline functions (no variant exists, no environment variable is read).
#include "crc32c_diag.inc"

namespace {
thread_local std::string g_last_error;

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), int(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  g_last_error = buf;
  return code;
}

#define KVSEP_HIP(call)                                              \
  do {                                                               \
    hipError_t _e = (call);                                          \
    if (_e != hipSuccess) return set_err(KVSEP_EHIP, #call, _e);     \
  } while (0)

int upload_tables(kvsep_crc32c_ctx* c) {
  DevTables h;
  gf2::byte_tables(gf2::zero_bytes_map(1024), &h.z1024[0][0]);
  gf2::byte_tables(gf2::zero_bytes_map(4), &h.z4[0][0]);
  for (int j = 0; j < 6; ++j) gf2::byte_tables(gf2::zero_bytes_map(16ull << j), &h.ztree[j][0][0]);
  for (uint32_t b = 0; b < 256; ++b) h.byte1[b] = gf2::byte_table_entry(b);
  gf2::byte_tables(gf2::zero_bytes_map(c->piece_bytes), &h.zpiece[0][0]);
  for (int k = 0; k < 3; ++k) gf2::byte_tables(gf2::zero_bytes_map(kSmallPiece << k), &h.zsmall[k][0][0]);
  gf2::byte_tables(gf2::zero_bytes_map(kNarrowRow), &h.znarrow[0][0]);
  gf2::x2n_table(h.x2n);
  gf2::xinv_table(h.xinv);
  if (!c->d_tabs) KVSEP_HIP(hipMalloc(&c->d_tabs, sizeof(DevTables)));
  KVSEP_HIP(hipMemcpy(c->d_tabs, &h, sizeof(DevTables), hipMemcpyHostToDevice));
  return KVSEP_OK;
}

// Wait until the scratch's previous user (on whatever stream) is done with it -- before a realloc.
int quiesce(Scratch& sc) {
  if (sc.used && sc.last_use) KVSEP_HIP(hipEventSynchronize(sc.last_use));
  return KVSEP_OK;
}
}  // namespace

// ---- DevBuf (kvsep_internal.h): the one place a scratch array is allocated, freed or given a capacity
template <typename T, bool kAlways, typename U>
void kvsep::DevBuf<T, kAlways, U>::drop() {
  hipFree(p);
  hipFree(q);
  p = nullptr;
  q = nullptr;
  cap = 0;
}

template <typename T, bool kAlways, typename U>
int kvsep::DevBuf<T, kAlways, U>::alloc(uint64_t need, uint64_t np, uint64_t nq) {
  hipError_t e = np ? hipMalloc(&p, np * sizeof(T)) : hipSuccess;
  if (e == hipSuccess && nq) e = hipMalloc(&q, nq * sizeof(U));
  if (e != hipSuccess) {
    drop();
    return set_err(KVSEP_EHIP, "hipMalloc of a scratch array", e);
  }
  cap = need;
  return KVSEP_OK;
}

template <typename T, bool kAlways, typename U>
int kvsep::DevBuf<T, kAlways, U>::ensure(Scratch& sc, uint64_t need, bool capturing, const char* what, uint64_t np,
                                         uint64_t nq) {
  if (holds(need)) return KVSEP_OK;
  if (capturing) return set_err(KVSEP_EINVAL, what);
  int rc = quiesce(sc);
  if (rc) return rc;
  drop();
  return alloc(need, np, nq);
}

namespace {
void free_plan(Scratch& sc) {
  sc.plan_blocks.drop();
  sc.plan_pieces.drop();
  sc.scan_tmp.drop();
}

// The scratch's cross-stream event, made on first use (kvsep_crc32c_reserve makes it for capture sets).
int ensure_event(Scratch& sc) {
  if (!sc.last_use) KVSEP_HIP(hipEventCreateWithFlags(&sc.last_use, hipEventDisableTiming));
  return KVSEP_OK;
}

// Order this call behind the scratch's previous user when it ran on another stream.
int acquire(Scratch& sc, hipStream_t s) {
  int rc = ensure_event(sc);
  if (rc) return rc;
  if (sc.used && sc.last_stream != s) KVSEP_HIP(hipStreamWaitEvent(s, sc.last_use, 0));
  return KVSEP_OK;
}

int release(Scratch& sc, hipStream_t s) {
  KVSEP_HIP(hipEventRecord(sc.last_use, s));
  sc.last_stream = s;
  sc.used = true;
  return KVSEP_OK;
}

// The verify form's device words (allocated once per scratch -- kvsep_crc32c_reserve does it for capture sets): on the
// first 128-B line the result words of a call whose caller passes none; then the accumulators eager calls post to and
// reset (PiecesArgs::vacc: the lowest-block word and the final arrival word, then 8 shard arrival words, each group on
// a line of its own), which must start in their reset state: ~0 (no mismatch), 0 (nothing arrived, none bad).  Eager
// calls on one scratch are ordered one after another by its events, so one set serves them all; captured calls publish
// through verdict slots instead (ensure_vslot), which hold no state from one call to the next.
constexpr uint32_t kVaccSetWords = kVaccStride * (1 + kVaccShards);
unsigned long long* vacc_set(Scratch& sc) { return sc.verify.p + kVaccStride; }

int ensure_verify(Scratch& sc) {
  if (sc.verify.p) return KVSEP_OK;
  std::vector<unsigned long long> init(kVaccStride + kVaccSetWords, 0ull);
  init[0] = ~0ull;             // default first_bad
  init[kVaccStride] = ~0ull;   // the set's vacc[0]
  int rc = sc.verify.alloc(init.size(), init.size());
  if (rc) return rc;
  KVSEP_HIP(hipMemcpy(sc.verify.p, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  sc.vacc_dirty = false;
  return KVSEP_OK;
}

// Verdict slots of captured verify calls: one per workgroup of the CRC kernel (num_cus) and of the combine kernel.
uint32_t vslots_needed(const kvsep_crc32c_ctx* c) { return uint32_t(c->num_cus) + kCombineMaxGrid; }

// (Only kvsep_crc32c_reserve sizes them, on a scratch no call is using: no quiesce, no capture path.)
int ensure_vslot(Scratch& sc, uint32_t n) {
  if (sc.vslot.cap >= n) return KVSEP_OK;
  sc.vslot.drop();
  return sc.vslot.alloc(n, 2 * uint64_t(n));
}

// The work counter of the guided schedule: allocated once per scratch, never under capture.
int ensure_counter(Scratch& sc, bool capturing = false) {
  if (sc.counter.p) return KVSEP_OK;
  if (capturing) return set_err(KVSEP_EINVAL, "graph capture needs kvsep_crc32c_reserve first");
  return sc.counter.alloc(4, 4);
}

// Puts the eager accumulator set back in its reset state, in stream order (two memsets).  Needed after an eager call
// that failed once its CRC kernel was enqueued: the kernel's posts stay in the set, and with no publishing kernel after
// them nothing resets it -- the next verdict would inherit a stale count and first_bad.  The failed call
// marks the set (vacc_dirty) and the next eager verify call on the scratch resets it first.  Captured calls never need
// this: their slots are overwritten whole by every replay.
int reset_vacc(Scratch& sc, hipStream_t s) {
  unsigned long long* v = vacc_set(sc);
  KVSEP_HIP(hipMemsetAsync(v, 0, kVaccSetWords * 8, s));
  KVSEP_HIP(hipMemsetAsync(v, 0xff, 8, s));
  sc.vacc_dirty = false;
  return KVSEP_OK;
}

// What each form's arrays are sized for and by: the capacity in the form's own unit, the refusal of a captured call
// that kvsep_crc32c_reserve did not size the capture set for, and the elements of each array.
int ensure_sst(Scratch& sc, uint64_t count, bool capturing = false) {
  return sc.sst.ensure(sc, count, capturing, "SST verify under capture needs kvsep_crc32c_reserve first", count, count);
}

// The list forms' tile arrays (crc32c_verdicts.inc): one total and one base per kListTile blocks.
int ensure_list(Scratch& sc, uint64_t count, bool capturing = false) {
  const uint64_t nt = list_tile_count(count);
  return sc.tiles.ensure(sc, nt, capturing,
                         "a captured list call larger than kvsep_crc32c_reserve sized its capture set for", nt, nt);
}

int ensure_offsets(Scratch& sc, uint64_t count, bool capturing = false) {
  return sc.off.ensure(sc, count, capturing,
                       "a captured offsets pass larger than kvsep_crc32c_reserve sized its capture set for", count,
                       offsets::scratch_words(count));
}

int ensure_log(Scratch& sc, uint64_t nblocks, bool capturing = false) {
  return sc.log.ensure(sc, nblocks, capturing,
                       "a captured log read larger than kvsep_crc32c_reserve sized its capture set for",
                       logrun::scratch_words(nblocks));
}

int ensure_chain(Scratch& sc, uint64_t cap, bool capturing = false) {
  return sc.chain.ensure(sc, cap, capturing,
                         "a captured chains pass larger than kvsep_crc32c_reserve sized its capture set for",
                         chain::scratch_words(cap));
}

// One word per record and one per fragment slot, one of each at least.
int ensure_logw(Scratch& sc, uint64_t n, bool capturing = false) {
  return sc.logw.ensure(sc, n, capturing,
                        "a captured log frame larger than kvsep_crc32c_reserve sized its capture set for", n ? n : 1,
                        n ? n : 1);
}

int ensure_sstidx(Scratch& sc, uint64_t runs, bool capturing = false) {
  return sc.sstidx.ensure(sc, runs, capturing,
                          "a captured SST index walk larger than kvsep_crc32c_reserve sized its capture set for",
                          sst::scratch_words(runs));
}

int ensure_sstw(Scratch& sc, uint64_t count, bool capturing = false) {
  return sc.sstw.ensure(sc, count, capturing,
                        "a captured SST index build larger than kvsep_crc32c_reserve sized its capture set for",
                        sstw::scratch_words(count));
}

// What a list form adds to its verify call: bad_idx[0, min(nbad, bad_cap)) and / or ok[0, count).
struct ListOut {
  uint64_t* bad_idx;
  uint64_t bad_cap;
  uint8_t* ok;
};

// The list pass over the CRCs a call just wrote.  nbad: the call's verdict word, already ordered before this on the
// stream (null: none, every kernel runs in full).  bad_cap == 0 needs no tile arrays: only ok[] is written.
int launch_list(Scratch& sc, hipStream_t s, bool capturing, const uint32_t* out, const uint32_t* stored,
                const uint64_t* nbad, const ListOut& l, uint64_t count) {
  if (!count || (!l.bad_cap && !l.ok)) return KVSEP_OK;
  const uint64_t nt = list_tile_count(count);
  const auto* nb = reinterpret_cast<const unsigned long long*>(nbad);
  if (l.bad_cap) {
    int rc = ensure_list(sc, count, capturing);
    if (rc) return rc;
  }
  verdict_tile_count_kernel<<<unsigned(nt), kListThreads, 0, s>>>(out, stored, count, nb, l.ok,
                                                         l.bad_cap ? sc.tiles.p : nullptr);
  KVSEP_HIP(hipGetLastError());
  if (!l.bad_cap) return KVSEP_OK;
  verdict_tile_scan_kernel<<<1, kListThreads, 0, s>>>(sc.tiles.p, sc.tiles.q, uint32_t(nt), nb);
  KVSEP_HIP(hipGetLastError());
  verdict_scatter_kernel<<<unsigned(nt), kListThreads, 0, s>>>(out, stored, count, nb, sc.tiles.q, l.bad_idx, l.bad_cap);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

// Where a verify call put its count: the caller's word, or the scratch's own when the caller passed none
// (launch_batch_body).
const uint64_t* verdict_nbad(const Scratch& sc, const uint64_t* first_bad, const uint64_t* nbad) {
  return first_bad && nbad ? nbad : reinterpret_cast<const uint64_t*>(sc.verify.p + 1);
}

// Room for a plan of `count` blocks and `pieces` entries (plan_size.h: pieces_needed of a call, pieces_reserved of a
// reservation).
int ensure_plan(Scratch& sc, uint64_t count, uint64_t pieces, bool capturing = false) {
  // hipcub's scan takes an int item count; piece and block indices are u32 in the kernels
  if (count > 0x7fffffffull) return set_err(KVSEP_EINVAL, "more than 2^31 - 1 blocks in one batch that needs a plan");
  if (pieces > 0xffffffffull) return set_err(KVSEP_EINVAL, "batch too large for u32 piece indices");
  if (sc.plan_blocks.holds(count) && sc.plan_pieces.holds(pieces)) return KVSEP_OK;
  if (capturing)
    return set_err(KVSEP_EINVAL, "a captured planned batch larger than kvsep_crc32c_reserve sized its capture set for");
  // both dimensions grow together, neither shrinks: the three buffers are dropped and allocated as one
  const uint64_t nc = std::max(count, sc.plan_blocks.cap), np = std::max(pieces, sc.plan_pieces.cap);
  int rc = quiesce(sc);
  if (rc) return rc;
  free_plan(sc);
  rc = sc.plan_blocks.alloc(nc, nc, nc + 1);
  if (!rc) rc = sc.plan_pieces.alloc(np, np, np);
  size_t tb = 0;
  if (!rc && hipcub::DeviceScan::InclusiveSum(nullptr, tb, sc.plan_blocks.p, sc.plan_blocks.q + 1, int(nc),
                                              hipStream_t(0)) != hipSuccess)
    rc = set_err(KVSEP_EHIP, "hipcub::DeviceScan::InclusiveSum (temporary storage query)");
  if (!rc) rc = sc.scan_tmp.alloc(tb, tb);
  if (rc) free_plan(sc);
  return rc;
}

// What a batch call runs as (route.h): the decision is made there, from the context's settings alone, and the launch,
// ensure_plan_for, kvsep_crc32c_plan_query and kvsep_crc32c_kernel_name all read this one Route.
route::Route route_of(const kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  return route::decide(c->settings(), count, total_bytes, max_len, diag_narrow(c));  // (KVSEP_DIAG build only: KVSEP_NARROW)
}

hipEvent_t take_event(kvsep_crc32c_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

template <bool P, bool D, bool V>
void launch_pieces_v(const kvsep_crc32c_ctx* c, unsigned grid, hipStream_t s, const PiecesArgs& a) {
  // Default (1): 8-wave workgroups (2 waves per SIMD, up to 256 VGPRs), 4-row groups, non-temporal loads, next
  // item staged ahead.  On one MI355X, interleaved in one process (tools/ab_variants.py), 8 waves beat 16 waves
  // by 1.5-2 % on 1 MiB blocks and by 4-5 % on the Zipf batch; 12 waves sit between.  (A 3-slot ring of row groups,
  // 8 rows in flight, was tried and measured -2 to -7 %: the extra VGPRs cost LDS-lookup overlap; so was staging items
  // two ahead, -1.5 % on the Zipf batch.)  Only the default is compiled into the shipped library; the A/B and ablation
  // variants live in crc32c_diag.inc, compiled into the KVSEP_DIAG tools build only.
  constexpr int T = kWgThreads;
  if (V) {  // the verify form: the shipped configuration only
    crc32c_pieces_kernel<P, D, 4, true, true, T, true, true><<<grid, T, 0, s>>>(a);
    return;
  }
  if (diag_launch_pieces<P, D>(c, grid, s, a)) return;  // KVSEP_DIAG build only
  crc32c_pieces_kernel<P, D, 4, true, true, T><<<grid, T, 0, s>>>(a);
}

template <bool V>
void launch_pieces_vv(const kvsep_crc32c_ctx* c, bool planned, bool dyn, unsigned grid, hipStream_t s,
                      const PiecesArgs& a) {
  if (planned) {
    if (dyn) launch_pieces_v<true, true, V>(c, grid, s, a);
    else launch_pieces_v<true, false, V>(c, grid, s, a);
  } else {
    if (dyn) launch_pieces_v<false, true, V>(c, grid, s, a);
    else launch_pieces_v<false, false, V>(c, grid, s, a);
  }
}

void launch_pieces(const kvsep_crc32c_ctx* c, bool planned, bool dyn, bool verify, unsigned grid, hipStream_t s,
                   const PiecesArgs& a) {
  if (verify) launch_pieces_vv<true>(c, planned, dyn, grid, s, a);
  else launch_pieces_vv<false>(c, planned, dyn, grid, s, a);
}

// The narrow forms (route.h), each with its verify form; `threads` is the route's, the template's own workgroup.
template <bool V>
void launch_narrow_v(route::Form form, bool init, unsigned grid, unsigned threads, hipStream_t s, const PiecesArgs& a) {
  using route::Form;
  switch (form) {
    case Form::Narrow8: crc32c_narrow_kernel<4, true, 512, true, true, LdsFull, V><<<grid, threads, 0, s>>>(a); break;
    case Form::Claim: crc32c_narrow_claim_kernel<4, 512, V, true, 8, kClaimLean><<<grid, threads, 0, s>>>(a); break;
    case Form::Claim16: crc32c_narrow_claim_kernel<4, 512, V, true, 16><<<grid, threads, 0, s>>>(a); break;
    case Form::Coop:
      if (init) crc32c_narrow_coop_kernel<V, true><<<grid, threads, 0, s>>>(a);
      else crc32c_narrow_coop_kernel<V, false><<<grid, threads, 0, s>>>(a);
      break;
    case Form::Sorted: crc32c_narrow_sorted_kernel<4, true, 1024, V><<<grid, threads, 0, s>>>(a); break;
    default: crc32c_narrow_kernel<4, true, 1024, false, true, LdsFull, V><<<grid, threads, 0, s>>>(a); break;
  }
}

void launch_narrow(const route::Route& r, bool verify, bool init, unsigned grid, hipStream_t s, const PiecesArgs& a) {
  if (verify) launch_narrow_v<true>(r.form, init, grid, r.threads, s, a);
  else launch_narrow_v<false>(r.form, init, grid, r.threads, s, a);
}

int launch_batch_in(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, const void* base,
                    const uint64_t* off, const uint64_t* len, const uint32_t* init, const uint32_t* expect,
                    uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count, uint64_t total_bytes,
                    uint64_t max_len);

// Is `s` capturing, and if so which capture set do its calls run on: the one this capture already holds, else the first
// free one.  No free set is an error at capture time (KVSEP_EINVAL), never a shared set.
int stream_scratch(kvsep_crc32c_ctx* c, hipStream_t s, Scratch& eager, bool* capturing, Scratch** out) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  KVSEP_HIP(hipStreamGetCaptureInfo(s, &cap, &id));
  *capturing = cap != hipStreamCaptureStatusNone;
  *out = &eager;
  if (!*capturing) return KVSEP_OK;
  for (auto& k : c->caps)
    if (k->held && k->id == id) {
      *out = &k->sc;
      return KVSEP_OK;
    }
  for (auto& k : c->caps)
    if (!k->held) {
      k->held = true;
      k->id = id;
      *out = &k->sc;
      return KVSEP_OK;
    }
  return set_err(KVSEP_EINVAL, c->caps.empty()
                                   ? "graph capture needs kvsep_crc32c_reserve first (it sizes the capture sets)"
                                   : "every capture set of this context is held by an earlier graph: "
                                     "kvsep_crc32c_reserve_captures for more, or kvsep_crc32c_release_captures once "
                                     "those graphs are destroyed");
}

// The scratch the calls on `s` run on, checked to hold what `needs(sc, capturing)` asks for: a captured call that was
// not reserved for is refused and an eager one allocates, before anything is enqueued.  (A capture that claimed a set
// keeps it when the needs refuse.)  The caller holds a DeviceGuard.
template <typename Needs>
int sized_scratch(kvsep_crc32c_ctx* c, hipStream_t s, Scratch& eager, Needs needs, bool* capturing, Scratch** psc) {
  int rc = stream_scratch(c, s, eager, capturing, psc);
  return rc ? rc : needs(**psc, *capturing);
}

// That check alone, for a composite call whose later steps bracket their own scratch: it refuses before its first step
// enqueues anything.  The caller holds the context's mutex.
template <typename Needs>
int check_scratch(kvsep_crc32c_ctx* c, hipStream_t s, Needs needs) {
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  bool capturing = false;
  Scratch* psc = nullptr;
  return sized_scratch(c, s, c->sc, needs, &capturing, &psc);
}

// Every use of a Scratch goes through this bracket.  Under stream capture (hipGraph) the call only
// records its nodes, on its capture's own set (stream_scratch): the cross-stream scratch events are skipped (a captured
// wait on an event recorded outside the capture is not allowed) and nothing is allocated -- kvsep_crc32c_reserve sized
// the set.  Calls captured into one graph share its set, so they must be ordered within the graph (captured on one
// stream, or joined).  An eager call sizes the scratch (`needs`), orders itself behind the scratch's previous user
// (acquire), enqueues `body(sc, capturing)` and records the scratch's event (release) -- after a failed body too, so
// that whatever it enqueued stays ordered before the scratch's next user.  The needs run before acquire: acquire only
// creates the event and enqueues a wait on `s`, and a need that reallocates synchronises the host on that same event
// (quiesce), so the order of the two makes no difference, and a refusal has enqueued nothing.  The caller holds the
// context's mutex; `eager` is the context's scratch, or a staging slot's own.
template <typename Needs, typename Body>
int with_scratch(kvsep_crc32c_ctx* c, hipStream_t s, Scratch& eager, Needs needs, Body body) {
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  bool capturing = false;
  Scratch* psc = nullptr;
  int rc = sized_scratch(c, s, eager, needs, &capturing, &psc);
  if (!rc && !capturing) rc = acquire(*psc, s);
  if (rc) return rc;
  rc = body(*psc, capturing);
  if (capturing) return rc;
  const int rel = release(*psc, s);
  return rc ? rc : rel;
}

// The plan of a checksum step inside a larger call, when its route takes one: sized with the call's other needs.
int ensure_plan_for(kvsep_crc32c_ctx* c, Scratch& sc, uint64_t count, uint64_t total_bytes, uint64_t max_len,
                    bool capturing) {
  const route::Route r = route_of(c, count, total_bytes, max_len);
  if (!r.planned) return KVSEP_OK;
  return ensure_plan(sc, count, r.pieces_needed, capturing);
}

int launch_batch(kvsep_crc32c_ctx* c, Scratch& eager, hipStream_t s, const void* base, const uint64_t* off,
                 const uint64_t* len, const uint32_t* init, const uint32_t* expect, uint32_t* out, uint64_t* first_bad,
                 uint64_t* nbad, uint64_t count, uint64_t total_bytes, uint64_t max_len,
                 const ListOut* list = nullptr) {
  if (!base || !off || !len || !out) return set_err(KVSEP_EINVAL, "null pointer argument");
  // block indices travel as u32 through the descriptor windows and the piece table
  if (count > 0xffffffffull) return set_err(KVSEP_EINVAL, "more than 2^32 - 1 blocks in one batch");
  return with_scratch(
      c, s, eager,
      [&](Scratch& sc, bool capturing) { return list && list->bad_cap ? ensure_list(sc, count, capturing) : KVSEP_OK; },
      [&](Scratch& sc, bool capturing) {
        int rc = launch_batch_in(c, sc, s, capturing, base, off, len, init, expect, out, first_bad, nbad, count,
                                 total_bytes, max_len);
        if (!rc && list)
          rc = launch_list(sc, s, capturing, out, expect, verdict_nbad(sc, first_bad, nbad), *list, count);
        return rc;
      });
}

int launch_batch_body(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, PiecesArgs& a,
                      const void* base, const uint64_t* off, const uint64_t* len, const uint32_t* init,
                      const uint32_t* expect, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                      uint64_t total_bytes, uint64_t max_len);

int launch_batch_in(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, const void* base,
                    const uint64_t* off, const uint64_t* len, const uint32_t* init, const uint32_t* expect,
                    uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count, uint64_t total_bytes,
                    uint64_t max_len) {
  PiecesArgs a{};
  if (expect) {
    if (capturing) {  // verdict slots (reserved with the capture set), published by the reduce kernel
      if (!sc.verify.p || sc.vslot.cap < vslots_needed(c))
        return set_err(KVSEP_EINVAL, "verify under capture needs kvsep_crc32c_reserve first");
      a.vslot = sc.vslot.p;
    } else {
      int rc = ensure_verify(sc);
      if (rc) return rc;
      if (sc.vacc_dirty) {
        rc = reset_vacc(sc, s);
        if (rc) return rc;
      }
      a.vacc = vacc_set(sc);  // the accumulators, in their reset state: the kernels publish the verdict
    }
  }
  const int rc = launch_batch_body(c, sc, s, capturing, a, base, off, len, init, expect, out, first_bad, nbad, count,
                                   total_bytes, max_len);
  if (rc && expect && !capturing) sc.vacc_dirty = true;  // a kernel may have posted to the set: reset it first next time
  return rc;
}

int launch_batch_body(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, PiecesArgs& a,
                      const void* base, const uint64_t* off, const uint64_t* len, const uint32_t* init,
                      const uint32_t* expect, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                      uint64_t total_bytes, uint64_t max_len) {
  const route::Route route = route_of(c, count, total_bytes, max_len);
  const bool planned = route.planned;
  a.base = static_cast<const uint8_t*>(base);
  a.off = off;
  a.len = len;
  a.init = init;
  a.out = out;
  a.count = count;
  a.piece_bytes = route.piece.bytes;
  a.zpiece = !planned ? nullptr : route.piece.table < 0 ? &c->d_tabs->zpiece[0][0] : &c->d_tabs->zsmall[route.piece.table][0][0];
  a.tabs = c->d_tabs;
  if (expect) {
    if (!first_bad || !nbad) {
      first_bad = reinterpret_cast<uint64_t*>(sc.verify.p);
      nbad = reinterpret_cast<uint64_t*>(sc.verify.p + 1);
    }
    if (count == 0) {  // nothing to check, no CRC kernel: the verdict is "none" (first_bad = ~0, nbad = 0)
      start_words_kernel<<<1, 64, 0, s>>>(nullptr, reinterpret_cast<unsigned long long*>(first_bad),
                                          reinterpret_cast<unsigned long long*>(nbad));
      KVSEP_HIP(hipGetLastError());
    }
  }
  a.expect = expect;
  a.first_bad = reinterpret_cast<unsigned long long*>(first_bad);
  a.nbad = reinterpret_cast<unsigned long long*>(nbad);
  // The verify form's compare runs inside the CRC kernels (and the combine kernel for split blocks).  Only the narrow
  // variants of the KVSEP_DIAG tools build fall back to a separate pass (crc32c_diag.inc: diag_verify_finish).
  if (count == 0) return KVSEP_OK;
  const bool dyn = route.dyn;
  a.static_contig = c->static_contig;
  a.guided_div = 0;  // adaptive (crc32c_pieces_kernel)
  a.guided_cap = 0;
  if (dyn) {
    int rc = ensure_counter(sc, capturing);
    if (rc) return rc;
    a.work_counter = sc.counter.p;
  }
  // The start-state words (pstart[0], the guided counter) are written by a kernel of the call, never by a memset node
  // (see crc32c_plan_count_kernel).
  if (planned) {
    int rc = ensure_plan(sc, count, route.pieces_needed, capturing);
    if (rc) return rc;
    a.pstart = sc.plan_blocks.q;
    a.pblk = sc.plan_pieces.p;
    a.partial = sc.plan_pieces.q;
    a.max_pieces = sc.plan_pieces.cap;
    const unsigned nb = unsigned((count + 255) / 256);
    crc32c_plan_count_kernel<<<nb, 256, 0, s>>>(len, count, a.piece_bytes, sc.plan_blocks.p, sc.plan_blocks.q,
                                                dyn ? sc.counter.p : nullptr);
    KVSEP_HIP(hipGetLastError());
    size_t tb = sc.scan_tmp.cap;
    KVSEP_HIP(hipcub::DeviceScan::InclusiveSum(sc.scan_tmp.p, tb, sc.plan_blocks.p, sc.plan_blocks.q + 1, int(count), s));
    crc32c_plan_expand_kernel<<<nb, 256, 0, s>>>(sc.plan_blocks.q, count, sc.plan_pieces.cap, sc.plan_pieces.p);
    KVSEP_HIP(hipGetLastError());
  } else {
    a.max_pieces = count;
    if (dyn) {
      start_words_kernel<<<1, 64, 0, s>>>(sc.counter.p, nullptr, nullptr);
      KVSEP_HIP(hipGetLastError());
    }
  }
  const unsigned grid = unsigned(c->num_cus);  // one workgroup per CU, persistent
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->timing) {
    e0 = take_event(c);
    e1 = take_event(c);
    if (e0 && e1) KVSEP_HIP(hipEventRecord(e0, s));
  }
  a.hint = route.hint;
  if (route.form != route::Form::Wide) {
    KVSEP_HIP(diag_verify_words(route, s, a));  // KVSEP_DIAG build only: a narrow variant's verdict words
    if (!diag_launch_narrow(route, grid, s, a))  // KVSEP_DIAG build only: a narrow variant in place of the form
      launch_narrow(route, expect != nullptr, init != nullptr, grid, s, a);
  } else {
    launch_pieces(c, planned, dyn, expect != nullptr, grid, s, a);
  }
  KVSEP_HIP(hipGetLastError());
  if (c->inject_failure) {  // fault injection (tests): fail between the CRC kernel and the combine kernel
    c->inject_failure = false;
    if (e0) c->ev_pool.push_back(e0);  // the timing pair is not recorded: back to the pool
    if (e1) c->ev_pool.push_back(e1);
    return set_err(KVSEP_EHIP, "injected failure after the CRC kernel (kvsep_crc32c_ctx_inject_failure)");
  }
  if (c->timing && e0 && e1) {
    KVSEP_HIP(hipEventRecord(e1, s));
    c->ev_pending.emplace_back(e0, e1);
  }
  const unsigned cgrid = route.combine_grid;
  if (planned) {
    a.vslot_base = grid;  // a captured verify call: the combine kernel's slots follow the CRC kernel's
    if (expect) crc32c_combine_kernel<true><<<cgrid, 256, 0, s>>>(a);
    else crc32c_combine_kernel<false><<<cgrid, 256, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
  }
  if (expect && a.vslot) {  // a captured verify call's verdict from its slots
    verify_slots_reduce_kernel<<<1, 256, 0, s>>>(a.vslot, grid + cgrid,
                                                 reinterpret_cast<unsigned long long*>(first_bad),
                                                 reinterpret_cast<unsigned long long*>(nbad));
    KVSEP_HIP(hipGetLastError());
  }
  KVSEP_HIP(diag_verify_finish(route, s, a));  // KVSEP_DIAG build only: the verdict of a variant without a compare
  return KVSEP_OK;
}
}  // namespace

namespace kvsep {
int device_batch_locked(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, const void* base, const uint64_t* off,
                        const uint64_t* len, const uint32_t* init, uint32_t* out, uint64_t count,
                        uint64_t total_bytes, uint64_t max_len) {
  return launch_batch(c, sc, s, base, off, len, init, nullptr, out, nullptr, nullptr, count, total_bytes, max_len);
}

void free_scratch(Scratch& sc) {
  if (sc.used && sc.last_use) (void)hipEventSynchronize(sc.last_use);
  sc.each_buf([](auto& b) { b.drop(); });
  if (sc.last_use) (void)hipEventDestroy(sc.last_use);
  sc = Scratch();
}
HostStaging& ctx_staging(kvsep_crc32c_ctx* c) { return c->staging; }
std::mutex& ctx_mutex(kvsep_crc32c_ctx* c) { return c->mu; }
int ctx_device(kvsep_crc32c_ctx* c) { return c->device; }
int ctx_host_node(kvsep_crc32c_ctx* c) { return c->host_node; }
uint64_t ctx_piece_bytes(kvsep_crc32c_ctx* c) { return c->piece_bytes; }
void set_last_error(const char* msg) { g_last_error = msg; }
}  // namespace kvsep

extern "C" {

int kvsep_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int kvsep_crc32c_ctx_create(int device, kvsep_crc32c_ctx** out) {
  if (!out) return set_err(KVSEP_EINVAL, "out is null");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0)
    return set_err(KVSEP_ENODEV, "no HIP device with that ordinal");
  hipDeviceProp_t prop;
  KVSEP_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::string m = std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only";
    return set_err(KVSEP_ENODEV, m.c_str());
  }
  DeviceGuard dg(device);
  KVSEP_HIP(dg.err);
  auto* c = new kvsep_crc32c_ctx();
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  c->host_node = kvsep_device_numa_node(device);
  diag_env(c);  // tools build only: no environment variable reaches the shipped library's kernel choice
  int rc = upload_tables(c);
  if (rc) {
    delete c;
    return rc;
  }
  *out = c;
  return KVSEP_OK;
}

void kvsep_crc32c_ctx_destroy(kvsep_crc32c_ctx* c) {
  if (!c) return;
  DeviceGuard dg(c->device);
  hipDeviceSynchronize();
  free_scratch(c->sc);
  for (auto& k : c->caps) free_scratch(k->sc);
  hipFree(c->d_tabs);
  for (auto& p : c->ev_pending) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
  for (auto e : c->ev_pool) hipEventDestroy(e);
  release_staging(c->staging);
  diag_forget(c);  // KVSEP_DIAG build only
  delete c;
}

int kvsep_crc32c_ctx_set_piece_bytes(kvsep_crc32c_ctx* c, uint64_t piece_bytes) {
  if (!c || piece_bytes < 1024 || piece_bytes % 1024) return set_err(KVSEP_EINVAL, "piece_bytes must be a multiple of 1 KiB");
  std::lock_guard<std::mutex> g(c->mu);
  // a captured graph holds this piece size and the table image it reads (Z_piece): it would replay wrong
  for (auto& k : c->caps)
    if (k->held) return set_err(KVSEP_EINVAL, "set_piece_bytes with captured graphs held: kvsep_crc32c_release_captures first");
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  KVSEP_HIP(hipDeviceSynchronize());
  c->piece_bytes = piece_bytes;
  c->piece_auto = false;
  free_plan(c->sc);  // piece tables depend on piece_bytes (device already idle)
  for (auto& sc : c->staging.scratch) free_plan(sc);
  for (auto& k : c->caps) free_plan(k->sc);  // none is held (above); kvsep_crc32c_reserve sizes them again
  return upload_tables(c);
}

int kvsep_crc32c_ctx_set_schedule(kvsep_crc32c_ctx* c, int dynamic) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  c->dynamic = dynamic < 0 ? -1 : (dynamic == 1 ? 1 : 0);
  c->static_contig = dynamic == 2 ? 0 : 1;
  return KVSEP_OK;
}

int kvsep_crc32c_ctx_set_kernel(kvsep_crc32c_ctx* c, int kernel) {
  if (!c || kernel < 0 || kernel > 8) return set_err(KVSEP_EINVAL, "kernel must be 0..8");
  std::lock_guard<std::mutex> g(c->mu);
  c->kernel = kernel;
  return KVSEP_OK;
}

int kvsep_crc32c_ctx_set_host_node(kvsep_crc32c_ctx* c, int node) {
  if (!c || node < -1) return set_err(KVSEP_EINVAL, "node must be >= -1");
  std::lock_guard<std::mutex> g(c->mu);
  c->host_node = node;
  return KVSEP_OK;
}

int kvsep_crc32c_ctx_inject_failure(kvsep_crc32c_ctx* c) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  // a test hook (csrc/kvsep_testing.h, not the public header): inert unless the test environment asks for it
  const char* on = std::getenv("KVSEP_TEST_HOOKS");
  if (!on || std::strcmp(on, "1") != 0) return set_err(KVSEP_EINVAL, "fault injection needs KVSEP_TEST_HOOKS=1");
  std::lock_guard<std::mutex> g(c->mu);
  c->inject_failure = true;
  return KVSEP_OK;
}

}  // extern "C"

namespace {
// Everything a call of up to count blocks / total_bytes could allocate on this scratch: the plan is sized for the
// worst of the piece sizes a smaller batch can pick, and for the SST read check's extra byte per block
// (plan::pieces_reserved).
int reserve_scratch(kvsep_crc32c_ctx* c, Scratch& sc, uint64_t count, uint64_t total_bytes) {
  int rc = ensure_counter(sc);
  if (!rc) rc = ensure_verify(sc);
  if (!rc) rc = ensure_event(sc);
  if (!rc) rc = ensure_sst(sc, count);
  if (!rc) rc = ensure_vslot(sc, vslots_needed(c));
  if (!rc) rc = ensure_list(sc, count);
  if (!rc) rc = ensure_offsets(sc, count);
  if (!rc) rc = ensure_log(sc, count);
  if (!rc) rc = ensure_chain(sc, count);
  if (!rc) rc = ensure_logw(sc, count);
  if (!rc) rc = ensure_sstidx(sc, sst::runs_for(sst::runs_reserved(count), 0));
  if (!rc) rc = ensure_sstw(sc, count);
  if (rc) return rc;
  return ensure_plan(sc, count, plan::pieces_reserved(c->piece_bytes, c->piece_auto, c->num_cus, count, total_bytes));
}

// At least n capture sets, each free one sized for the context's largest reservation (held ones stay as their graph
// captured them).
int reserve_capture_sets(kvsep_crc32c_ctx* c, size_t n) {
  while (c->caps.size() < n) c->caps.emplace_back(new CaptureSet());
  for (auto& k : c->caps) {
    if (k->held) continue;
    int rc = reserve_scratch(c, k->sc, c->res_count, c->res_bytes);
    if (rc) return rc;
  }
  return KVSEP_OK;
}
}  // namespace

extern "C" {

int kvsep_crc32c_reserve(kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  // everything a later call could allocate: on the context's own scratch (eager calls), and on every free capture set
  // (the calls of a graph capture, which must not allocate)
  int rc = reserve_scratch(c, c->sc, count, total_bytes);
  if (rc) return rc;
  c->res_count = std::max(c->res_count, count);
  c->res_bytes = std::max(c->res_bytes, total_bytes);
  return reserve_capture_sets(c, std::max(c->caps.size(), kDefaultCaptureSets));
}

int kvsep_crc32c_reserve_captures(kvsep_crc32c_ctx* c, int nsets) {
  if (!c || nsets < 0 || nsets > 4096) return set_err(KVSEP_EINVAL, "nsets must be 0..4096");
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  return reserve_capture_sets(c, size_t(nsets));
}

int kvsep_crc32c_release_captures(kvsep_crc32c_ctx* c) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  for (auto& k : c->caps) k->held = false;
  return KVSEP_OK;
}

int kvsep_crc32c_capture_sets(kvsep_crc32c_ctx* c, int* held) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  int h = 0;
  for (auto& k : c->caps) h += k->held ? 1 : 0;
  if (held) *held = h;
  return int(c->caps.size());
}

int kvsep_crc32c_ctx_set_timing(kvsep_crc32c_ctx* c, int enable) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  c->timing = enable != 0;
  return KVSEP_OK;
}

int kvsep_crc32c_ctx_get_timing(kvsep_crc32c_ctx* c, double* total_ms, uint64_t* launches) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  double ms = 0;
  uint64_t n = 0;
  for (auto& p : c->ev_pending) {
    KVSEP_HIP(hipEventSynchronize(p.second));
    float t = 0;
    KVSEP_HIP(hipEventElapsedTime(&t, p.first, p.second));
    ms += t;
    ++n;
    c->ev_pool.push_back(p.first);
    c->ev_pool.push_back(p.second);
  }
  c->ev_pending.clear();
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return KVSEP_OK;
}

int kvsep_crc32c_batch_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                              const uint64_t* len, const uint32_t* init, uint32_t* out, uint64_t count,
                              uint64_t total_bytes, uint64_t max_len) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  return launch_batch(c, c->sc, static_cast<hipStream_t>(stream), base, off, len, init, nullptr, out, nullptr,
                      nullptr, count, total_bytes, max_len);
}

int kvsep_crc32c_verify_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                               const uint64_t* len, const uint32_t* init, const uint32_t* expected_masked,
                               uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                               uint64_t total_bytes, uint64_t max_len) {
  if (!c || !expected_masked) return set_err(KVSEP_EINVAL, "null ctx or expected_masked");
  std::lock_guard<std::mutex> g(c->mu);
  return launch_batch(c, c->sc, static_cast<hipStream_t>(stream), base, off, len, init, expected_masked, out,
                      first_bad, nbad, count, total_bytes, max_len);
}

int kvsep_crc32c_verify_list_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                                    const uint64_t* len, const uint32_t* init, const uint32_t* expected_masked,
                                    uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t* bad_idx,
                                    uint64_t bad_cap, uint8_t* ok, uint64_t count, uint64_t total_bytes,
                                    uint64_t max_len) {
  if (!c || !expected_masked) return set_err(KVSEP_EINVAL, "kvsep_crc32c_verify_list_device: null ctx or expected_masked");
  if (!bad_idx && bad_cap) return set_err(KVSEP_EINVAL, "kvsep_crc32c_verify_list_device: null bad_idx with bad_cap > 0");
  std::lock_guard<std::mutex> g(c->mu);
  const ListOut l{bad_idx, bad_cap, ok};
  return launch_batch(c, c->sc, static_cast<hipStream_t>(stream), base, off, len, init, expected_masked, out,
                      first_bad, nbad, count, total_bytes, max_len, &l);
}

int kvsep_log_verify_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                            const uint64_t* len, const uint32_t* stored, uint8_t* ok, uint64_t count,
                            uint64_t total_bytes, uint64_t max_len) {
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_log_verify_device: null ctx");
  if (!base || !off || !len || !stored || !ok) return set_err(KVSEP_EINVAL, "kvsep_log_verify_device: null argument");
  if (count > 0xffffffffull) return set_err(KVSEP_EINVAL, "kvsep_log_verify_device: more than 2^32 - 1 records");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the CRCs go to the scratch's u32 word per block (the SST read check's array: kvsep_crc32c_reserve sizes it), then
  // ok[i] = Mask(crc) == stored[i], which is db/log_reader.cc:250-258's crc == Unmask(stored)
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return ensure_sst(sc, count, capturing); },
      [&](Scratch& sc, bool capturing) {
        int rc = launch_batch_in(c, sc, s, capturing, base, off, len, nullptr, nullptr, sc.sst.q, nullptr, nullptr,
                                 count, total_bytes, max_len);
        if (!rc) rc = launch_list(sc, s, capturing, sc.sst.q, stored, nullptr, ListOut{nullptr, 0, ok}, count);
        return rc;
      });
}

int kvsep_fill_splitmix64_device(void* stream, void* dst, uint64_t nbytes, uint64_t seed, uint64_t stream_offset) {
  if (!dst && nbytes) return set_err(KVSEP_EINVAL, "null dst");
  if (!nbytes) return KVSEP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = 256 * 8;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (stream_offset & 15) == 0) {
    const uint64_t n16 = nbytes / 16;
    if (n16) fill_splitmix_fast_kernel<<<grid, 256, 0, s>>>(static_cast<uint4*>(dst), n16, seed, stream_offset / 8);
    const uint64_t rest = nbytes - n16 * 16;
    if (rest)
      fill_splitmix_bytes_kernel<<<1, 64, 0, s>>>(static_cast<uint8_t*>(dst) + n16 * 16, rest, seed,
                                                  stream_offset + n16 * 16);
  } else {
    fill_splitmix_bytes_kernel<<<grid, 256, 0, s>>>(static_cast<uint8_t*>(dst), nbytes, seed, stream_offset);
  }
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

int kvsep_sst_trailers_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                              const uint64_t* len, const uint8_t* types, uint32_t* masked_out, uint64_t count,
                              uint64_t total_bytes, uint64_t max_len) {
  if (!c || !types || !masked_out) return set_err(KVSEP_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = launch_batch(c, c->sc, s, base, off, len, nullptr, nullptr, masked_out, nullptr, nullptr, count,
                        total_bytes, max_len);
  if (rc || !count) return rc;
  sst_trailer_finish_kernel<<<unsigned((count + 255) / 256), 256, 0, s>>>(masked_out, types, masked_out, count,
                                                                          c->d_tabs);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

}  // extern "C"

namespace {
// The batched combine on `s`: one launch, no scratch (crc32c_concat.inc).  The caller holds the context's mutex and has
// checked the arguments.
int launch_concat(kvsep_crc32c_ctx* c, hipStream_t s, const uint32_t* seg_crc, const uint64_t* seg_len,
                  const uint64_t* first, const uint32_t* init, uint32_t* out, uint64_t count, uint64_t nseg) {
  if (!count) return KVSEP_OK;
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  crc32c_concat_kernel<<<unsigned(concat::grid_for(count)), kConcatThreads, 0, s>>>(seg_crc, seg_len, first, init, out,
                                                                                    count, nseg, c->d_tabs);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

int concat_args(const char* who, kvsep_crc32c_ctx* c, const void* seg_a, const void* seg_b, const uint64_t* first,
                const uint32_t* out, uint64_t count, uint64_t nseg) {
  const char* what = !c                                 ? "null ctx"
                     : count && (!first || !out)        ? "null first or out"
                     : nseg && (!seg_a || !seg_b)       ? "null segment array"
                     : count > 0xffffffffull            ? "more than 2^32 - 1 blocks in one batch"
                                                        : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}

// The gather form on `s`: the segment pass is the batched form itself, on whatever route its hints pick; the combine
// follows on the stream.  The caller holds the context's mutex and has checked the arguments.
int launch_gather(kvsep_crc32c_ctx* c, hipStream_t s, const void* base, const uint64_t* seg_off,
                  const uint64_t* seg_len, const uint64_t* first, const uint32_t* init, uint32_t* seg_crc, uint32_t* out,
                  uint64_t count, uint64_t nseg, uint64_t total_bytes, uint64_t max_len) {
  if (nseg) {
    int rc = launch_batch(c, c->sc, s, base, seg_off, seg_len, nullptr, nullptr, seg_crc, nullptr, nullptr, nseg,
                          total_bytes, max_len);
    if (rc) return rc;
  }
  return launch_concat(c, s, seg_crc, seg_len, first, init, out, count, nseg);
}

// The gather-copy on `s`: one launch, no scratch (crc32c_pack.inc).  The first part of the grid gives every
// pack::kShortBlocks blocks a wavefront, the second every chunk of pack::kChunkBlocks blocks a team of workgroups --
// about four workgroups per CU in all for a small batch (pack::team_size).  The caller holds the context's mutex and has
// checked the arguments.
template <typename F>
int launch_pack(kvsep_crc32c_ctx* c, hipStream_t s, PackArgs a) {
  if (!a.count) return KVSEP_OK;
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  a.short_wgs = pack::short_wgs(a.count);
  a.team = pack::team_size(a.count, 4u * uint32_t(c->num_cus > 0 ? c->num_cus : 256));
  const uint64_t grid = a.short_wgs + pack::chunk_count(a.count) * a.team;  // < 2^29 for count < 2^32
  crc32c_pack_kernel<F><<<unsigned(grid), kPackThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

int pack_args(const char* who, kvsep_crc32c_ctx* c, const uint64_t* seg_off, const uint64_t* seg_len,
              const uint64_t* first, const void* dst, const uint64_t* dst_off, uint64_t count, uint64_t nseg) {
  const char* what = !c                                       ? "null ctx"
                     : count && (!first || !dst || !dst_off)  ? "null first, dst or offset array"
                     : nseg && (!seg_off || !seg_len)         ? "null segment array"
                     : count > 0xffffffffull                  ? "more than 2^32 - 1 blocks in one batch"
                                                              : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}
}  // namespace

extern "C" {

int kvsep_crc32c_concat_device(kvsep_crc32c_ctx* c, void* stream, const uint32_t* seg_crc, const uint64_t* seg_len,
                               const uint64_t* first, const uint32_t* init, uint32_t* out, uint64_t count,
                               uint64_t nseg) {
  int rc = concat_args("kvsep_crc32c_concat_device", c, seg_crc, seg_len, first, out, count, nseg);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  return launch_concat(c, static_cast<hipStream_t>(stream), seg_crc, seg_len, first, init, out, count, nseg);
}

int kvsep_crc32c_gather_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* seg_off,
                               const uint64_t* seg_len, const uint64_t* first, const uint32_t* init, uint32_t* seg_crc,
                               uint32_t* out, uint64_t count, uint64_t nseg, uint64_t total_bytes, uint64_t max_len) {
  int rc = concat_args("kvsep_crc32c_gather_device", c, seg_off, seg_len, first, out, count, nseg);
  if (rc) return rc;
  if (nseg && !seg_crc) return set_err(KVSEP_EINVAL, "kvsep_crc32c_gather_device: null seg_crc");
  std::lock_guard<std::mutex> g(c->mu);
  return launch_gather(c, static_cast<hipStream_t>(stream), base, seg_off, seg_len, first, init, seg_crc, out, count,
                       nseg, total_bytes, max_len);
}

int kvsep_crc32c_pack_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* seg_off,
                             const uint64_t* seg_len, const uint64_t* first, void* dst, uint64_t dst_bytes,
                             const uint64_t* dst_off, uint64_t count, uint64_t nseg) {
  int rc = pack_args("kvsep_crc32c_pack_device", c, seg_off, seg_len, first, dst, dst_off, count, nseg);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  return launch_pack<PackPlain>(c, static_cast<hipStream_t>(stream),
                                PackArgs{static_cast<const uint8_t*>(base), seg_off, seg_len, first,
                                         static_cast<uint8_t*>(dst), dst_bytes, dst_off, count, nseg, nullptr, nullptr,
                                         0, 0});
}

int kvsep_vlog_frame_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* seg_off,
                            const uint64_t* seg_len, const uint64_t* first, uint32_t* seg_crc, uint32_t* crc_out,
                            void* dst, uint64_t dst_bytes, const uint64_t* rec_off, uint64_t count, uint64_t nseg,
                            uint64_t total_bytes, uint64_t max_len) {
  int rc = pack_args("kvsep_vlog_frame_device", c, seg_off, seg_len, first, dst, rec_off, count, nseg);
  if (rc) return rc;
  if ((nseg && !seg_crc) || (count && !crc_out))
    return set_err(KVSEP_EINVAL, "kvsep_vlog_frame_device: null seg_crc or crc_out");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = launch_gather(c, s, base, seg_off, seg_len, first, nullptr, seg_crc, crc_out, count, nseg, total_bytes, max_len);
  if (rc) return rc;
  return launch_pack<PackVlog>(c, s,
                               PackArgs{static_cast<const uint8_t*>(base), seg_off, seg_len, first,
                                        static_cast<uint8_t*>(dst), dst_bytes, rec_off, count, nseg, crc_out, nullptr, 0,
                                        0});
}

int kvsep_sst_frame_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                           const uint64_t* len, const uint8_t* types, uint32_t* masked_out, void* dst,
                           uint64_t dst_bytes, const uint64_t* blk_off, uint64_t count, uint64_t total_bytes,
                           uint64_t max_len) {
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_frame_device: null ctx");
  if (!types || !masked_out || (count && (!off || !len || !dst || !blk_off)))
    return set_err(KVSEP_EINVAL, "kvsep_sst_frame_device: null argument");
  if (count > 0xffffffffull)
    return set_err(KVSEP_EINVAL, "kvsep_sst_frame_device: more than 2^32 - 1 blocks in one batch");
  int rc = kvsep_sst_trailers_device(c, stream, base, off, len, types, masked_out, count, total_bytes, max_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  // block i is segment i: no first[]
  return launch_pack<PackSst>(c, static_cast<hipStream_t>(stream),
                              PackArgs{static_cast<const uint8_t*>(base), off, len, nullptr, static_cast<uint8_t*>(dst),
                                       dst_bytes, blk_off, count, count, masked_out, types, 0, 0});
}

}  // extern "C"

namespace {
// The SST read check, and its list form when `list` is given (the stored words are the ones the prep kernel extracts).
// The caller holds the context's mutex.
int sst_verify_locked(kvsep_crc32c_ctx* c, void* stream, const void* file_base, const uint64_t* off,
                      const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                      uint64_t total_bytes, uint64_t max_len, const ListOut* list) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_scratch(
      c, s, c->sc,
      [&](Scratch& sc, bool capturing) {  // (kvsep_crc32c_reserve sizes the SST arrays too)
        int rc = ensure_sst(sc, count, capturing);
        if (!rc && list && list->bad_cap) rc = ensure_list(sc, count, capturing);
        return rc;
      },
      [&](Scratch& sc, bool capturing) {
        if (!count) {
          // No handle: the verdict is "none", posted here.  launch_batch_in takes a call for a verify by its stored-word
          // array, and a scratch that never held SST arrays has none for count 0.
          if (first_bad || nbad) {
            start_words_kernel<<<1, 64, 0, s>>>(nullptr, reinterpret_cast<unsigned long long*>(first_bad),
                                                reinterpret_cast<unsigned long long*>(nbad));
            KVSEP_HIP(hipGetLastError());
          }
          return KVSEP_OK;
        }
        {
          sst_verify_prep_kernel<<<unsigned((count + 255) / 256), 256, 0, s>>>(
              static_cast<const uint8_t*>(file_base), off, len, sc.sst.p, sc.sst.q, count);
          KVSEP_HIP(hipGetLastError());
        }
        int rc = launch_batch_in(c, sc, s, capturing, file_base, off, sc.sst.p, nullptr, sc.sst.q, out, first_bad, nbad,
                                 count, total_bytes + count, max_len ? max_len + 1 : 0);
        if (!rc && list)
          rc = launch_list(sc, s, capturing, out, sc.sst.q, verdict_nbad(sc, first_bad, nbad), *list, count);
        return rc;
      });
}

int sst_verify_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, const uint64_t* off,
                      const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                      uint64_t total_bytes, uint64_t max_len, const ListOut* list) {
  std::lock_guard<std::mutex> g(c->mu);
  return sst_verify_locked(c, stream, file_base, off, len, out, first_bad, nbad, count, total_bytes, max_len, list);
}

// ---- the offsets pass and the salvage forms built on it (crc32c_offsets.inc)

// What an offsets pass is asked for; the scratch pointers are filled in by launch_offsets_in.
struct OffsetsCall {
  const uint64_t* seg_len;
  const uint64_t* first;
  const uint8_t* keep;
  const uint64_t* keep_before;
  uint64_t head, tail, start, max_size;
  uint64_t* dst_off;
  uint64_t* end;
  uint64_t* nkept;
  uint64_t count, nseg;
};

// The three kernels on `s`, on a scratch the caller has acquired and sized (ensure_offsets).  An empty batch runs the
// write kernel alone, which then touches no scratch.
int launch_offsets_in(Scratch& sc, hipStream_t s, const OffsetsCall& o) {
  const uint64_t nt = offsets::tile_count(o.count);
  OffsetsArgs a{};
  a.seg_len = o.seg_len;
  a.first = o.first;
  a.keep = o.keep;
  a.keep_before = reinterpret_cast<const unsigned long long*>(o.keep_before);
  a.head = o.head, a.tail = o.tail, a.start = o.start, a.max_size = o.max_size;
  a.count = o.count, a.nseg = o.nseg;
  a.dst_off = o.dst_off, a.end = o.end, a.nkept = o.nkept;
  if (nt) {
    const offsets::TileWords w = offsets::tile_words(nt);
    a.ext = sc.off.p;
    a.tile_sum = sc.off.q + w.sum;
    a.tile_kept = sc.off.q + w.kept;
    a.tile_base = sc.off.q + w.base;
    a.grand = sc.off.q + w.grand;
    offsets_tile_sum_kernel<<<unsigned(nt), offsets::kThreads, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
    offsets_tile_scan_kernel<<<1, offsets::kScanThreads, 0, s>>>(a.tile_sum, a.tile_kept, a.tile_base, a.grand, nt);
    KVSEP_HIP(hipGetLastError());
  }
  offsets_write_kernel<<<unsigned(nt ? nt : 1), offsets::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

// What an offsets pass over `count` blocks needs.
auto offsets_needs(uint64_t count) {
  return [=](Scratch& sc, bool capturing) { return ensure_offsets(sc, count, capturing); };
}

// The offsets pass as a call of its own, in its own scratch bracket.  `then`, when given, is enqueued inside the bracket
// (a copy that reads the pass's scratch).  The caller holds the context's mutex.
template <typename Then>
int launch_offsets(kvsep_crc32c_ctx* c, hipStream_t s, const OffsetsCall& o, Then then) {
  return with_scratch(c, s, c->sc, offsets_needs(o.count), [&](Scratch& sc, bool) {
    const int rc = launch_offsets_in(sc, s, o);
    return rc ? rc : then(sc);
  });
}

int launch_offsets(kvsep_crc32c_ctx* c, hipStream_t s, const OffsetsCall& o) {
  return launch_offsets(c, s, o, [](Scratch&) { return KVSEP_OK; });
}

// Refusals shared by the offsets and salvage forms, before the context is looked at (so they hold on a machine with no
// device): both keep rules at once, more blocks than a u32 index, a missing output.
int offsets_args(const char* who, const void* keep, const void* keep_before, const void* dst_off, const void* end,
                 uint64_t count) {
  const char* what = keep && keep_before           ? "both keep and keep_before given: one keep rule at most"
                     : count > 0xffffffffull       ? "more than 2^32 - 1 blocks in one batch"
                     : !end || (count && !dst_off) ? "null dst_off or end"
                                                   : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}
}  // namespace

extern "C" {

int kvsep_crc32c_offsets_device(kvsep_crc32c_ctx* c, void* stream, const uint64_t* seg_len, const uint64_t* first,
                                const uint8_t* keep, const uint64_t* keep_before, uint64_t head_bytes,
                                uint64_t tail_bytes, uint64_t start, uint64_t* dst_off, uint64_t* end, uint64_t* nkept,
                                uint64_t count, uint64_t nseg) {
  const char* who = "kvsep_crc32c_offsets_device";
  int rc = offsets_args(who, keep, keep_before, dst_off, end, count);
  if (rc) return rc;
  if (nseg && !seg_len) return set_err(KVSEP_EINVAL, "kvsep_crc32c_offsets_device: null seg_len");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_crc32c_offsets_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  return launch_offsets(c, static_cast<hipStream_t>(stream),
                        OffsetsCall{seg_len, first, keep, keep_before, head_bytes, tail_bytes, start, ~uint64_t(0),
                                    dst_off, end, nkept, count, nseg});
}

int kvsep_crc32c_salvage_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                                const uint64_t* len, const uint8_t* keep, const uint64_t* keep_before, void* dst,
                                uint64_t dst_bytes, uint64_t* dst_off, uint64_t* end, uint64_t* nkept, uint64_t count) {
  int rc = offsets_args("kvsep_crc32c_salvage_device", keep, keep_before, dst_off, end, count);
  if (rc) return rc;
  if (count && (!off || !len || !dst)) return set_err(KVSEP_EINVAL, "kvsep_crc32c_salvage_device: null off, len or dst");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_crc32c_salvage_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = launch_offsets(c, s, OffsetsCall{len, nullptr, keep, keep_before, 0, 0, 0, ~uint64_t(0), dst_off, end, nkept,
                                        count, count});
  if (rc) return rc;
  // block i is segment i: no first[]; a dropped block's kSkip lies in no destination (pack::fits)
  return launch_pack<PackPlain>(c, s,
                                PackArgs{static_cast<const uint8_t*>(base), off, len, nullptr,
                                         static_cast<uint8_t*>(dst), dst_bytes, dst_off, count, count, nullptr, nullptr,
                                         0, 0});
}

int kvsep_sst_salvage_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, const uint64_t* off,
                             const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint8_t* ok,
                             void* dst, uint64_t dst_bytes, uint64_t* dst_off, uint64_t* end, uint64_t* nkept,
                             uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  int rc = offsets_args("kvsep_sst_salvage_device", nullptr, nullptr, dst_off, end, count);
  if (rc) return rc;
  if (!file_base || !off || !len || !out || !ok || (count && !dst))
    return set_err(KVSEP_EINVAL, "kvsep_sst_salvage_device: null argument");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_salvage_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // refused before anything is enqueued (the read check makes its own checks first thing, too)
  rc = check_scratch(c, s, offsets_needs(count));
  if (rc) return rc;
  const ListOut l{nullptr, 0, ok};
  rc = sst_verify_locked(c, stream, file_base, off, len, out, first_bad, nbad, count, total_bytes, max_len, &l);
  if (rc) return rc;
  // A kept block's extent is its bytes plus the 5-byte trailer that follows them in the file, a dropped one's is 0: the
  // pass's extent array is the length array of the copy, which therefore runs inside the pass's scratch bracket.
  return launch_offsets(c, s, OffsetsCall{len, nullptr, ok, nullptr, 0, 5, 0, ~uint64_t(0), dst_off, end, nkept, count,
                                          count},
                        [&](Scratch& sc) {
                          return launch_pack<PackPlain>(
                              c, s,
                              PackArgs{static_cast<const uint8_t*>(file_base), off,
                                       reinterpret_cast<const uint64_t*>(sc.off.p), nullptr,
                                       static_cast<uint8_t*>(dst), dst_bytes, dst_off, count, count, nullptr, nullptr, 0,
                                       0});
                        });
}

int kvsep_vlog_frame_auto_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* seg_off,
                                 const uint64_t* seg_len, const uint64_t* first, uint32_t* seg_crc, uint32_t* crc_out,
                                 void* dst, uint64_t dst_bytes, uint64_t start, uint64_t* rec_off, uint64_t* end,
                                 uint64_t count, uint64_t nseg, uint64_t total_bytes, uint64_t max_len) {
  int rc = offsets_args("kvsep_vlog_frame_auto_device", nullptr, nullptr, rec_off, end, count);
  if (rc) return rc;
  rc = pack_args("kvsep_vlog_frame_auto_device", c, seg_off, seg_len, first, dst, rec_off, count, nseg);
  if (rc) return rc;
  if ((nseg && !seg_crc) || (count && !crc_out))
    return set_err(KVSEP_EINVAL, "kvsep_vlog_frame_auto_device: null seg_crc or crc_out");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // refused before anything is enqueued
  rc = check_scratch(c, s, offsets_needs(count));
  if (rc) return rc;
  rc = launch_gather(c, s, base, seg_off, seg_len, first, nullptr, seg_crc, crc_out, count, nseg, total_bytes, max_len);
  if (rc) return rc;
  // a payload the header's LE32 length cannot hold is refused as kvsep_vlog_frame_offsets refuses it: no offset for it
  // or for any record after it, *end = 2^64 - 1
  rc = launch_offsets(c, s, OffsetsCall{seg_len, first, nullptr, nullptr, 8, 0, start, 0xffffffffull, rec_off, end,
                                        nullptr, count, nseg});
  if (rc) return rc;
  return launch_pack<PackVlog>(c, s,
                               PackArgs{static_cast<const uint8_t*>(base), seg_off, seg_len, first,
                                        static_cast<uint8_t*>(dst), dst_bytes, rec_off, count, nseg, crc_out, nullptr, 0,
                                        0});
}

}  // extern "C"

namespace {
// ---- the log / MANIFEST reader on the device (crc32c_logwalk.inc)

struct LogWalkCall {
  const void* base;
  uint64_t n;
  uint64_t* off;
  uint64_t* len;
  uint32_t* stored;
  uint8_t* type;
  uint64_t cap;
  uint64_t* nrec;
};

struct LogAcceptCall {
  const void* base;
  uint64_t n;
  const uint64_t* off;
  const uint64_t* len;
  const uint8_t* type;
  const uint8_t* ok;
  const uint64_t* nrec;
  uint64_t cap;
  uint8_t* accept;
  uint8_t* gap;
  uint64_t* dropped;
  uint64_t* bad_length;
};

// Refusals before any device is touched.
int log_walk_args(const char* who, const kvsep_crc32c_ctx* c, const void* base, uint64_t n, uint64_t cap,
                  const void* nrec) {
  const char* what = !c                    ? "null ctx"
                     : !base && n          ? "null base with n != 0"
                     : !nrec               ? "null nrec"
                     : cap > 0xffffffffull ? "cap over 2^32 - 1"
                                           : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}

int log_accept_args(const char* who, const kvsep_crc32c_ctx* c, const LogAcceptCall& a) {
  int rc = log_walk_args(who, c, a.base, a.n, a.cap, a.nrec);
  if (rc) return rc;
  if (a.cap && (!a.off || !a.len || !a.type || !a.ok || !a.accept))
    return set_err(KVSEP_EINVAL, (std::string(who) + ": null off, len, type, ok or accept with cap != 0").c_str());
  return KVSEP_OK;
}

// The walk on a scratch the caller has acquired and sized: count, the offsets pass over the counts, fill.
int launch_log_walk_in(Scratch& sc, hipStream_t s, const LogWalkCall& w) {
  const uint64_t nb = logrun::block_count(w.n);
  LogWalkArgs a{};
  a.img = static_cast<const uint8_t*>(w.base);
  a.n = w.n, a.nblocks = nb;
  a.off = w.off, a.len = w.len, a.stored = w.stored, a.type = w.type;
  a.cap = w.cap;
  a.nrec = reinterpret_cast<const unsigned long long*>(w.nrec);
  const logrun::Words lw = logrun::words(nb);
  a.cnt = sc.log.p + lw.cnt;
  a.base = sc.log.p + lw.base;
  if (nb) {
    log_count_kernel<<<unsigned(logrun::grid_for(nb)), logrun::kThreads, 0, s>>>(a.img, a.n, nb, a.cnt);
    KVSEP_HIP(hipGetLastError());
  }
  // base[b] = the records before block b, *nrec = all of them: block b is "segment" b of cnt[], every block kept
  int rc = launch_offsets_in(sc, s,
                             OffsetsCall{reinterpret_cast<const uint64_t*>(a.cnt), nullptr, nullptr, nullptr, 0, 0, 0,
                                         ~uint64_t(0), reinterpret_cast<uint64_t*>(a.base), w.nrec, nullptr, nb, nb});
  if (rc) return rc;
  log_fill_kernel<<<unsigned(logrun::pad_grid(nb, w.cap)), logrun::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

// The accept pass on a scratch the caller has acquired and sized.
int launch_log_accept_in(Scratch& sc, hipStream_t s, const LogAcceptCall& w) {
  const uint64_t nb = logrun::block_count(w.n);
  LogAcceptArgs a{};
  a.img = static_cast<const uint8_t*>(w.base);
  a.n = w.n, a.nblocks = nb;
  a.off = w.off, a.len = w.len, a.type = w.type, a.ok = w.ok;
  a.nrec = reinterpret_cast<const unsigned long long*>(w.nrec);
  a.cap = w.cap;
  a.accept = w.accept, a.gap = w.gap, a.dropped = w.dropped, a.bad_length = w.bad_length;
  const logrun::Words lw = logrun::words(nb);
  a.stop = sc.log.p + lw.stop;
  a.first = sc.log.p + lw.first;
  a.state = sc.log.p + lw.state;
  a.cand = sc.log.p + lw.cand;
  a.drop = sc.log.p + lw.drop;
  a.badlen = sc.log.p + lw.badlen;
  if (nb) {
    log_block_kernel<<<unsigned(logrun::grid_for(nb)), logrun::kThreads, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
  }
  log_stop_kernel<<<logrun::kReduceGrid, logrun::kThreads, 0, s>>>(a.cand, nb, a.stop);
  KVSEP_HIP(hipGetLastError());
  log_accept_kernel<<<unsigned(logrun::pad_grid(nb, w.cap)), logrun::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  if (w.dropped || w.bad_length) {
    log_totals_kernel<<<logrun::kReduceGrid, logrun::kThreads, 0, s>>>(a.drop, a.badlen, nb, w.dropped, w.bad_length);
    KVSEP_HIP(hipGetLastError());
  }
  return KVSEP_OK;
}

// What a log call over an image of n bytes needs: the log words, the offsets pass over the blocks when it walks, and
// when it checks verify_count checksums their CRC words and plan -- refused with the rest, not between two enqueued
// steps.
auto log_needs(kvsep_crc32c_ctx* c, uint64_t n, bool walk, uint64_t verify_count) {
  return [=](Scratch& sc, bool capturing) {
    const uint64_t nb = logrun::block_count(n);
    int rc = ensure_log(sc, nb, capturing);
    if (!rc && walk) rc = ensure_offsets(sc, nb, capturing);
    if (!rc && verify_count) rc = ensure_sst(sc, verify_count, capturing);
    if (!rc && verify_count)
      rc = ensure_plan_for(c, sc, verify_count, n, logrun::kBlock - logrun::kTypeAt, capturing);
    return rc;
  };
}

// A log call as a call of its own, in its own scratch bracket.  The caller holds the context's mutex.
template <typename Body>
int launch_log(kvsep_crc32c_ctx* c, hipStream_t s, uint64_t n, bool walk, uint64_t verify_count, Body body) {
  return with_scratch(c, s, c->sc, log_needs(c, n, walk, verify_count), body);
}

// The walk, the checksum step and the accept pass of the read and records forms, on a scratch sized by log_needs.
int launch_log_read_in(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, const LogWalkCall& w,
                       const LogAcceptCall& acc, uint8_t* ok) {
  int r = launch_log_walk_in(sc, s, w);
  // the checksum step of kvsep_log_verify_device over all cap elements: the padding has length 0, Value("") = 0 and
  // Mask(0) != 0 = stored, so ok[] is 0 there
  if (!r && w.cap)
    r = launch_batch_in(c, sc, s, capturing, w.base, w.off, w.len, nullptr, nullptr, sc.sst.q, nullptr, nullptr, w.cap,
                        w.n, logrun::kBlock - logrun::kTypeAt);
  if (!r) r = launch_list(sc, s, capturing, sc.sst.q, w.stored, nullptr, ListOut{nullptr, 0, ok}, w.cap);
  if (!r) r = launch_log_accept_in(sc, s, acc);
  return r;
}
}  // namespace

extern "C" {

int kvsep_log_walk_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, uint64_t* off,
                          uint64_t* len, uint32_t* stored, uint8_t* type, uint64_t cap, uint64_t* nrec) {
  int rc = log_walk_args("kvsep_log_walk_device", c, base, n, cap, nrec);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LogWalkCall w{base, n, off, len, stored, type, cap, nrec};
  return launch_log(c, s, n, true, 0, [&](Scratch& sc, bool) { return launch_log_walk_in(sc, s, w); });
}

int kvsep_log_accept_gaps_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, const uint64_t* off,
                                 const uint64_t* len, const uint8_t* type, const uint8_t* ok, const uint64_t* nrec,
                                 uint64_t cap, uint8_t* accept, uint8_t* gap, uint64_t* dropped,
                                 uint64_t* bad_length_bytes) {
  const LogAcceptCall w{base, n, off, len, type, ok, nrec, cap, accept, gap, dropped, bad_length_bytes};
  int rc = log_accept_args("kvsep_log_accept_gaps_device", c, w);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return launch_log(c, s, n, false, 0, [&](Scratch& sc, bool) { return launch_log_accept_in(sc, s, w); });
}

int kvsep_log_read_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, uint64_t* off,
                          uint64_t* len, uint32_t* stored, uint8_t* type, uint8_t* ok, uint8_t* accept, uint8_t* gap,
                          uint64_t cap, uint64_t* nrec, uint64_t* dropped, uint64_t* bad_length_bytes) {
  const char* who = "kvsep_log_read_device";
  const LogAcceptCall acc{base, n, off, len, type, ok, nrec, cap, accept, gap, dropped, bad_length_bytes};
  int rc = log_accept_args(who, c, acc);
  if (rc) return rc;
  if (cap && !stored) return set_err(KVSEP_EINVAL, "kvsep_log_read_device: null stored with cap != 0");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LogWalkCall w{base, n, off, len, stored, type, cap, nrec};
  return launch_log(c, s, n, true, cap, [&](Scratch& sc, bool capturing) {
    return launch_log_read_in(c, sc, s, capturing, w, acc, ok);
  });
}

}  // extern "C"

namespace {
// ---- the value-log reader on the device (crc32c_vlogwalk.inc)

struct VlogWalkCall {
  const void* base;
  uint64_t n;
  uint64_t* off;
  uint64_t* len;
  uint32_t* stored;
  uint64_t cap;
  uint64_t* nrec;
  uint64_t* consumed;
};

// The walk on `s`: one launch, no scratch.
int launch_vlog_walk(hipStream_t s, const VlogWalkCall& w) {
  VlogWalkArgs a{};
  a.img = static_cast<const uint8_t*>(w.base);
  a.n = w.n;
  a.off = w.off, a.len = w.len, a.stored = w.stored;
  a.cap = w.cap;
  a.nrec = reinterpret_cast<unsigned long long*>(w.nrec);
  a.consumed = reinterpret_cast<unsigned long long*>(w.consumed);
  vlog_walk_kernel<<<1, vlogrun::kLanes, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

// What the read form's checksum step needs, stated before anything is enqueued: a captured call finds all of it in its
// capture set or is refused -- also when its cap is over what kvsep_crc32c_reserve sized the set for, which no array of
// this form would show (the CRCs go to the caller's array).
auto vlog_read_needs(kvsep_crc32c_ctx* c, uint64_t n, uint64_t cap, uint64_t max_len) {
  return [=](Scratch& sc, bool capturing) {
    if (!cap) return int(KVSEP_OK);
    if (capturing && (!sc.verify.p || sc.vslot.cap < vslots_needed(c) || !sc.sst.holds(cap)))
      return set_err(KVSEP_EINVAL, "a captured vlog read larger than kvsep_crc32c_reserve sized its capture set for");
    int rc = capturing ? KVSEP_OK : ensure_verify(sc);
    if (!rc && route_of(c, cap, n, max_len).dyn) rc = ensure_counter(sc, capturing);
    if (!rc) rc = ensure_plan_for(c, sc, cap, n, max_len, capturing);
    return rc;
  };
}
}  // namespace

extern "C" {

int kvsep_vlog_walk_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, uint64_t* off,
                           uint64_t* len, uint32_t* stored, uint64_t cap, uint64_t* nrec, uint64_t* consumed) {
  int rc = log_walk_args("kvsep_vlog_walk_device", c, base, n, cap, nrec);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  return launch_vlog_walk(static_cast<hipStream_t>(stream), VlogWalkCall{base, n, off, len, stored, cap, nrec, consumed});
}

int kvsep_vlog_read_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, uint64_t* off,
                           uint64_t* len, uint32_t* stored, uint32_t* crc, uint8_t* ok, uint64_t cap,
                           uint64_t max_len_hint, uint64_t* nrec, uint64_t* consumed, uint64_t* first_bad,
                           uint64_t* nbad, uint64_t* ngood, uint64_t* good_bytes, uint64_t* drop_bytes) {
  int rc = log_walk_args("kvsep_vlog_read_device", c, base, n, cap, nrec);
  if (rc) return rc;
  if (cap && (!off || !len || !stored || !crc))
    return set_err(KVSEP_EINVAL, "kvsep_vlog_read_device: null off, len, stored or crc with cap != 0");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t max_len = max_len_hint ? max_len_hint : n;
  const VlogWalkCall w{base, n, off, len, stored, cap, nrec, consumed};
  return with_scratch(c, s, c->sc, vlog_read_needs(c, n, cap, max_len), [&](Scratch& sc, bool capturing) -> int {
    int r = launch_vlog_walk(s, w);
    if (r) return r;
    VlogTotalsArgs t{};
    if (cap) {
      // kvsep_crc32c_verify_device over all cap elements: the padding is an empty block whose stored word is Mask(0),
      // which passes and is never dereferenced, so first_bad / nbad speak of records only
      uint64_t* fb = first_bad && nbad ? first_bad : reinterpret_cast<uint64_t*>(sc.verify.p);
      uint64_t* nb = first_bad && nbad ? nbad : reinterpret_cast<uint64_t*>(sc.verify.p + 1);
      r = launch_batch_in(c, sc, s, capturing, base, off, len, nullptr, stored, crc, fb, nb, cap, n, max_len);
      if (!r) r = launch_list(sc, s, capturing, crc, stored, nb, ListOut{nullptr, 0, ok}, cap);
      if (r) return r;
      t.first_bad_in = reinterpret_cast<const unsigned long long*>(fb);
      t.nbad_in = reinterpret_cast<const unsigned long long*>(nb);
    }
    t.nrec = reinterpret_cast<const unsigned long long*>(nrec);
    t.off = off, t.len = len, t.cap = cap;
    t.first_bad = reinterpret_cast<unsigned long long*>(first_bad);
    t.nbad = reinterpret_cast<unsigned long long*>(nbad);
    t.ngood = reinterpret_cast<unsigned long long*>(ngood);
    t.good_bytes = reinterpret_cast<unsigned long long*>(good_bytes);
    t.drop_bytes = reinterpret_cast<unsigned long long*>(drop_bytes);
    vlog_totals_kernel<<<1, vlogrun::kLanes, 0, s>>>(t);
    KVSEP_HIP(hipGetLastError());
    return KVSEP_OK;
  });
}

}  // extern "C"

namespace {
// ---- the SST table reader on the device (crc32c_sstindex.inc)

static_assert(sst::kOk == KVSEP_SST_OK && sst::kBadFooter == KVSEP_SST_BAD_FOOTER &&
                  sst::kIndexChecksum == KVSEP_SST_INDEX_CHECKSUM &&
                  sst::kIndexCompressed == KVSEP_SST_INDEX_COMPRESSED && sst::kBadRestarts == KVSEP_SST_BAD_RESTARTS &&
                  sst::kBadEntry == KVSEP_SST_BAD_ENTRY && sst::kBadHandle == KVSEP_SST_BAD_HANDLE &&
                  sst::kCap == KVSEP_SST_CAP,
              "sst_run.h restates the public status codes");
static_assert(sst::kSkip == offsets::kSkip && sst::kNone == offsets::kKeepAll, "the walk reads the offsets pass's marks");

struct SstWalkCall {
  const void* base;
  uint64_t n;
  const uint64_t* handle;   // device: index_off, index_len
  const uint64_t* handles;  // the table form: the footer's four (null: the walk alone)
  const uint32_t* crc;      // ... the index block's checksum as computed
  uint64_t* off;
  uint64_t* len;
  uint64_t cap;
  uint64_t* nblocks;
  uint32_t* status;
  bool keys = false;            // the keys walk: where each emitted entry's key lies in the image, and its length
  uint64_t* key_off = nullptr;
  uint64_t* key_len = nullptr;
};

// What an SST walk with `cap` slots over an image of n bytes needs: the index words, and the offsets pass over its runs.
int sst_walk_needs(Scratch& sc, bool capturing, uint64_t n, uint64_t cap) {
  int rc = ensure_sstidx(sc, sst::runs_for(sc.sstidx.cap, cap), capturing);
  if (!rc) rc = ensure_offsets(sc, sst::runs_used(sc.sstidx.cap, n), capturing);
  return rc;
}

// The walk on a scratch the caller has acquired and sized: count, stop, the offsets pass over the counts, fill.
int launch_sst_walk_in(Scratch& sc, hipStream_t s, const SstWalkCall& w) {
  const uint64_t runs = sst::runs_used(sc.sstidx.cap, w.n);  // sst_walk_needs made the capacity >= 1
  SstIndexArgs a{};
  a.img = static_cast<const uint8_t*>(w.base);
  a.n = w.n;
  a.handle = w.handle;
  a.runs = runs;
  a.handles = w.handles;
  a.crc = w.crc;
  a.stored = sc.sst.q;
  a.off = w.off, a.len = w.len, a.cap = w.cap;
  a.nblocks = reinterpret_cast<unsigned long long*>(w.nblocks);
  a.status = w.status;
  a.stop = sc.sstidx.p;
  a.cnt = sc.sstidx.p + sst::kStopWords;
  a.errbase = a.cnt + runs;
  a.wgstop = a.errbase + runs;
  const uint64_t nwg = sst::grid_for(runs);
  if (w.keys) sst_keys_count_kernel<<<unsigned(nwg), sst::kThreads, 0, s>>>(a);
  else sst_index_count_kernel<<<unsigned(nwg), sst::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  sst_index_stop_kernel<<<1, sst::kThreads, 0, s>>>(a.wgstop, nwg, a.errbase, a.stop);
  KVSEP_HIP(hipGetLastError());
  // base[r] = the entries before run r, *nblocks = all of them: run r is "segment" r of cnt[], kept up to the stop
  int rc = launch_offsets_in(sc, s,
                             OffsetsCall{reinterpret_cast<const uint64_t*>(a.cnt), nullptr, nullptr,
                                         reinterpret_cast<const uint64_t*>(a.stop), 0, 0, 0, ~uint64_t(0),
                                         reinterpret_cast<uint64_t*>(a.errbase), w.nblocks, nullptr, runs, runs});
  if (rc) return rc;
  if (w.keys)
    sst_keys_fill_kernel<<<unsigned(sst::pad_grid(runs, w.cap)), sst::kThreads, 0, s>>>(
        SstKeysArgs{a, w.key_off, w.key_len});
  else
    sst_index_fill_kernel<<<unsigned(sst::pad_grid(runs, w.cap)), sst::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}

// Refusals before the context or a device is touched.
int sst_walk_args(const char* who, const void* base, uint64_t n, const void* off, const void* len, uint64_t cap,
                  const void* nblocks, const void* status) {
  const char* what = !base && n                  ? "null file_base with n != 0"
                     : cap && (!off || !len)     ? "null off or len with cap != 0"
                     : !nblocks || !status       ? "null nblocks or status"
                     : cap > 0xffffffffull       ? "cap over 2^32 - 1"
                                                 : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}
// The whole-table verify (and, with key_off / key_len, its keys walk), as a step other forms share.
struct SstTableCall {
  const void* base;
  uint64_t n;
  uint64_t* off;
  uint64_t* len;
  uint64_t* key_off;  // null: the plain walk
  uint64_t* key_len;
  uint32_t* crc;
  uint64_t* first_bad;
  uint64_t* nbad;
  uint64_t* bad_idx;
  uint64_t bad_cap;
  uint8_t* ok;
  uint64_t cap, max_len_hint;
  uint64_t* nblocks;
  uint64_t* handles;
  uint32_t* status;
};

int sst_table_args(const char* who, const SstTableCall& t) {
  const std::string w(who);
  if (t.cap < 2) return set_err(KVSEP_EINVAL, (w + ": cap below 2 (the metaindex and index slots)").c_str());
  int rc = sst_walk_args(who, t.base, t.n, t.off, t.len, t.cap, t.nblocks, t.status);
  if (rc) return rc;
  if (!t.crc || !t.handles) return set_err(KVSEP_EINVAL, (w + ": null crc or handles").c_str());
  if (!t.bad_idx && t.bad_cap) return set_err(KVSEP_EINVAL, (w + ": null bad_idx with bad_cap > 0").c_str());
  return KVSEP_OK;
}

// The walk, and everything the two read checks and the list pass need, refused rather than between two enqueued steps.
int sst_table_needs(kvsep_crc32c_ctx* c, Scratch& sc, bool capturing, const SstTableCall& t) {
  const uint64_t hint1 = t.max_len_hint ? t.max_len_hint + 1 : 0;
  int rc = sst_walk_needs(sc, capturing, t.n, t.cap);
  if (!rc) rc = ensure_sst(sc, t.cap, capturing);
  if (!rc && t.bad_cap) rc = ensure_list(sc, t.cap, capturing);
  if (!rc && capturing && (!sc.verify.p || !sc.counter.p || sc.vslot.cap < vslots_needed(c)))
    rc = set_err(KVSEP_EINVAL, "verify under capture needs kvsep_crc32c_reserve first");
  if (!rc) rc = ensure_plan_for(c, sc, 1, t.n, 0, capturing);
  if (!rc) rc = ensure_plan_for(c, sc, t.cap, t.n + t.cap, hint1, capturing);
  return rc;
}

int launch_sst_table_in(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, const SstTableCall& t) {
  const auto* img = static_cast<const uint8_t*>(t.base);
  const uint64_t hint1 = t.max_len_hint ? t.max_len_hint + 1 : 0;
  sst_footer_kernel<<<1, sst::kFooterThreads, 0, s>>>(img, t.n, t.handles, t.status);
  KVSEP_HIP(hipGetLastError());
  // the read check of the index block alone: its checksum into crc[0], its stored word into the scratch
  sst_table_prep_kernel<<<1, sst::kThreads, 0, s>>>(
      SstPrepArgs{img, t.n, t.handles + 2, t.handles + 3, 1, nullptr, t.status, t.cap, sc.sst.p, sc.sst.q});
  KVSEP_HIP(hipGetLastError());
  int r = launch_batch_in(c, sc, s, capturing, t.base, t.handles + 2, sc.sst.p, nullptr, nullptr, t.crc, nullptr,
                          nullptr, 1, t.n, 0);
  if (r) return r;
  SstWalkCall w{t.base, t.n, t.handles + 2, t.handles, t.crc, t.off, t.len, t.cap, t.nblocks, t.status};
  w.keys = t.key_off != nullptr, w.key_off = t.key_off, w.key_len = t.key_len;
  r = launch_sst_walk_in(sc, s, w);
  if (r) return r;
  // the read check and the list pass over all cap slots: padding has length 0 and passes
  sst_table_prep_kernel<<<unsigned(sst::grid_for(t.cap)), sst::kThreads, 0, s>>>(
      SstPrepArgs{img, t.n, t.off, t.len, t.cap, reinterpret_cast<const unsigned long long*>(t.nblocks), t.status,
                  t.cap, sc.sst.p, sc.sst.q});
  KVSEP_HIP(hipGetLastError());
  r = launch_batch_in(c, sc, s, capturing, t.base, t.off, sc.sst.p, nullptr, sc.sst.q, t.crc, t.first_bad, t.nbad,
                      t.cap, t.n + t.cap, hint1);
  if (r) return r;
  return launch_list(sc, s, capturing, t.crc, sc.sst.q, verdict_nbad(sc, t.first_bad, t.nbad),
                     ListOut{t.bad_idx, t.bad_cap, t.ok}, t.cap);
}

// ---- the SST table writer on the device (crc32c_sstbuild.inc)

static_assert(sstw::kOk == KVSEP_SSTW_OK && sstw::kTooLarge == KVSEP_SSTW_TOO_LARGE &&
                  sstw::kNoRoom == KVSEP_SSTW_NO_ROOM && sstw::kSource == KVSEP_SSTW_SOURCE &&
                  sst::kSharedKey == KVSEP_SST_SHARED_KEY,
              "sstw_run.h and sst_run.h restate the public status codes");
static_assert(sstw::kSkip == offsets::kSkip && sstw::kSkip == KVSEP_OFFSET_SKIP, "the builder reads the offsets pass's marks");

struct SstBuildCall {
  const void* key_base;
  const uint64_t* key_off;
  const uint64_t* key_len;
  const uint64_t* blk_off;
  const uint64_t* blk_len;
  const uint8_t* keep;
  uint64_t count;
  void* dst;
  uint64_t dst_bytes;
  const uint64_t* at;
  uint64_t* out_len;
  uint32_t* status;
  uint64_t* table_bytes;   // non-null: the table form (metaindex block before, footer after)
  const uint32_t* source;  // the rewrite: the walk's status word
};

// The length hint of the builder's checksum: the block lies inside dst and stays below 2^32 bytes.
uint64_t sst_build_hint(uint64_t dst_bytes) { return std::min<uint64_t>(dst_bytes, sstw::kMaxBlock); }

int sst_build_needs(kvsep_crc32c_ctx* c, Scratch& sc, bool capturing, uint64_t count, uint64_t dst_bytes) {
  int rc = ensure_sstw(sc, count, capturing);
  if (!rc) rc = ensure_offsets(sc, count, capturing);
  if (!rc && capturing && !sc.counter.p) rc = set_err(KVSEP_EINVAL, "graph capture needs kvsep_crc32c_reserve first");
  if (!rc) rc = ensure_plan_for(c, sc, 1, sst_build_hint(dst_bytes), 0, capturing);
  return rc;
}

int sst_build_args(const char* who, const SstBuildCall& b) {
  const char* what = b.count && (!b.key_off || !b.key_len || !b.blk_off || !b.blk_len)
                         ? "null key or handle array with count != 0"
                     : !b.dst || !b.at || !b.out_len || !b.status ? "null dst, position, out_len or status"
                     : b.count > 0xffffffffull                    ? "more than 2^32 - 1 entries"
                                                                  : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}

// Mask(Extend(Value(the empty block), "\0", 1)): the table form's metaindex trailer word, computed once.
uint32_t sst_meta_masked() {
  static const uint32_t word = [] {
    char blk[sstw::kEmptyBlock + 1];
    for (uint32_t j = 0; j <= sstw::kEmptyBlock; ++j) blk[j] = char(sstw::meta_byte(j, 0));
    return kvsep_crc32c_mask(kvsep_crc32c_extend_host(0, blk, sizeof blk));
  }();
  return word;
}

// The builder on a scratch the caller has acquired and sized (sst_build_needs): the size kernel, the offsets pass twice
// (3 launches each), the fill kernel, the batched checksum over the one block, the tail kernel.
int launch_sst_build_in(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, bool capturing, const SstBuildCall& b) {
  const sstw::Slices sl = sstw::slices(b.count);
  SstBuildArgs a{};
  a.key_base = static_cast<const uint8_t*>(b.key_base);
  a.key_off = b.key_off, a.key_len = b.key_len, a.blk_off = b.blk_off, a.blk_len = b.blk_len, a.keep = b.keep;
  a.count = b.count;
  a.dst = static_cast<uint8_t*>(b.dst);
  a.dst_bytes = b.dst_bytes;
  a.at = reinterpret_cast<const unsigned long long*>(b.at);
  a.lead = b.table_bytes ? sstw::kMetaFramed : 0;
  a.trail = b.table_bytes ? sstw::kFooter : 0;
  a.source = b.source;
  a.size = sc.sstw.p + sl.size, a.flag = sc.sstw.p + sl.flag, a.pos = sc.sstw.p + sl.pos, a.rank = sc.sstw.p + sl.rank;
  a.words = sc.sstw.p + sl.words;
  a.out_len = b.out_len, a.status = b.status, a.table_bytes = b.table_bytes;
  a.meta_masked = sst_meta_masked();
  a.tabs = c->d_tabs;
  auto* words = reinterpret_cast<uint64_t*>(a.words);
  if (b.count) {
    sstw_size_kernel<<<unsigned(sstw::grid_for(b.count)), sstw::kThreads, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
  }
  int rc = launch_offsets_in(sc, s,
                             OffsetsCall{reinterpret_cast<const uint64_t*>(a.size), nullptr, nullptr, nullptr, 0, 0, 0,
                                         ~uint64_t(0), reinterpret_cast<uint64_t*>(a.pos),
                                         words + sstw::kEntriesBytes, nullptr, b.count, b.count});
  if (!rc)
    rc = launch_offsets_in(sc, s,
                           OffsetsCall{reinterpret_cast<const uint64_t*>(a.flag), nullptr, nullptr, nullptr, 0, 0, 0,
                                       ~uint64_t(0), reinterpret_cast<uint64_t*>(a.rank), words + sstw::kNKept, nullptr,
                                       b.count, b.count});
  if (rc) return rc;
  sstw_fill_kernel<<<unsigned(sstw::grid_for(b.count)), sstw::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  rc = launch_batch_in(c, sc, s, capturing, b.dst, words + sstw::kCrcOff, words + sstw::kCrcLen, nullptr, nullptr,
                       reinterpret_cast<uint32_t*>(words + sstw::kCrc), nullptr, nullptr, 1,
                       sst_build_hint(b.dst_bytes), 0);
  if (rc) return rc;
  sstw_tail_kernel<<<1, sstw::kTailThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}
}  // namespace

extern "C" {

int kvsep_sst_index_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, uint64_t n, const uint64_t* handle,
                           uint64_t* off, uint64_t* len, uint64_t cap, uint64_t* nblocks, uint32_t* status) {
  const char* who = "kvsep_sst_index_device";
  int rc = sst_walk_args(who, file_base, n, off, len, cap, nblocks, status);
  if (rc) return rc;
  if (!handle) return set_err(KVSEP_EINVAL, "kvsep_sst_index_device: null handle");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_index_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SstWalkCall w{file_base, n, handle, nullptr, nullptr, off, len, cap, nblocks, status};
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return sst_walk_needs(sc, capturing, n, cap); },
      [&](Scratch& sc, bool) { return launch_sst_walk_in(sc, s, w); });
}

int kvsep_sst_table_verify_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, uint64_t n, uint64_t* off,
                                  uint64_t* len, uint32_t* crc, uint64_t* first_bad, uint64_t* nbad, uint64_t* bad_idx,
                                  uint64_t bad_cap, uint8_t* ok, uint64_t cap, uint64_t max_len_hint, uint64_t* nblocks,
                                  uint64_t* handles, uint32_t* status) {
  const SstTableCall t{file_base, n,       off, len,          nullptr, nullptr, crc,    first_bad,
                       nbad,      bad_idx, bad_cap, ok, cap,     max_len_hint, nblocks, handles, status};
  int rc = sst_table_args("kvsep_sst_table_verify_device", t);
  if (rc) return rc;
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_table_verify_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return sst_table_needs(c, sc, capturing, t); },
      [&](Scratch& sc, bool capturing) { return launch_sst_table_in(c, sc, s, capturing, t); });
}

int kvsep_sst_index_keys_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, uint64_t n,
                                const uint64_t* handle, uint64_t* off, uint64_t* len, uint64_t* key_off,
                                uint64_t* key_len, uint64_t cap, uint64_t* nblocks, uint32_t* status) {
  const char* who = "kvsep_sst_index_keys_device";
  int rc = sst_walk_args(who, file_base, n, off, len, cap, nblocks, status);
  if (rc) return rc;
  if (!handle) return set_err(KVSEP_EINVAL, "kvsep_sst_index_keys_device: null handle");
  if (cap && (!key_off || !key_len))
    return set_err(KVSEP_EINVAL, "kvsep_sst_index_keys_device: null key_off or key_len with cap != 0");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_index_keys_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  SstWalkCall w{file_base, n, handle, nullptr, nullptr, off, len, cap, nblocks, status};
  w.keys = true, w.key_off = key_off, w.key_len = key_len;  // (null with cap == 0: nothing is stored)
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return sst_walk_needs(sc, capturing, n, cap); },
      [&](Scratch& sc, bool) { return launch_sst_walk_in(sc, s, w); });
}

int kvsep_sst_index_build_device(kvsep_crc32c_ctx* c, void* stream, const void* key_base, const uint64_t* key_off,
                                 const uint64_t* key_len, const uint64_t* blk_off, const uint64_t* blk_len,
                                 const uint8_t* keep, uint64_t count, void* dst, uint64_t dst_bytes, const uint64_t* at,
                                 uint64_t* out_len, uint32_t* status) {
  const SstBuildCall b{key_base, key_off, key_len, blk_off, blk_len, keep,    count,
                       dst,      dst_bytes, at,    out_len, status,  nullptr, nullptr};
  int rc = sst_build_args("kvsep_sst_index_build_device", b);
  if (rc) return rc;
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_index_build_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return sst_build_needs(c, sc, capturing, count, dst_bytes); },
      [&](Scratch& sc, bool capturing) { return launch_sst_build_in(c, sc, s, capturing, b); });
}

int kvsep_sst_table_finish_device(kvsep_crc32c_ctx* c, void* stream, const void* key_base, const uint64_t* key_off,
                                  const uint64_t* key_len, const uint64_t* blk_off, const uint64_t* blk_len,
                                  const uint8_t* keep, uint64_t count, void* dst, uint64_t dst_bytes,
                                  const uint64_t* data_end, uint64_t* index_len, uint64_t* table_bytes,
                                  uint32_t* status) {
  const SstBuildCall b{key_base, key_off,   key_len,  blk_off,   blk_len, keep,        count,
                       dst,      dst_bytes, data_end, index_len, status,  table_bytes, nullptr};
  int rc = sst_build_args("kvsep_sst_table_finish_device", b);
  if (rc) return rc;
  if (!table_bytes) return set_err(KVSEP_EINVAL, "kvsep_sst_table_finish_device: null table_bytes");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_table_finish_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return sst_build_needs(c, sc, capturing, count, dst_bytes); },
      [&](Scratch& sc, bool capturing) { return launch_sst_build_in(c, sc, s, capturing, b); });
}

int kvsep_sst_table_rewrite_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, uint64_t n, void* dst,
                                   uint64_t dst_bytes, uint64_t* off, uint64_t* len, uint64_t* key_off,
                                   uint64_t* key_len, uint32_t* crc, uint8_t* ok, uint64_t* dst_off, uint64_t cap,
                                   uint64_t max_len_hint, uint64_t* nblocks, uint64_t* nkept, uint64_t* handles,
                                   uint32_t* status, uint64_t* index_len, uint64_t* table_bytes, uint32_t* wstatus) {
  const char* who = "kvsep_sst_table_rewrite_device";
  const SstTableCall t{file_base, n,       off, len, key_off, key_len,      crc,     nullptr,
                       nullptr,   nullptr, 0,   ok,  cap,     max_len_hint, nblocks, handles, status};
  int rc = sst_table_args(who, t);
  if (rc) return rc;
  if (!key_off || !key_len || !ok || !dst_off || !dst || !index_len || !table_bytes || !wstatus)
    return set_err(KVSEP_EINVAL, "kvsep_sst_table_rewrite_device: null argument");
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_table_rewrite_device: null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // every need of every step, before anything is enqueued
  const auto needs = [&](Scratch& sc, bool capturing) {
    int r = sst_table_needs(c, sc, capturing, t);
    if (!r) r = sst_build_needs(c, sc, capturing, cap, dst_bytes);
    return r;
  };
  return with_scratch(c, s, c->sc, needs, [&](Scratch& sc, bool capturing) -> int {
    int r = launch_sst_table_in(c, sc, s, capturing, t);
    if (r) return r;
    const sstw::Slices sl = sstw::slices(cap);
    auto* keep = reinterpret_cast<uint8_t*>(sc.sstw.p + sl.keep);
    auto* words = reinterpret_cast<uint64_t*>(sc.sstw.p + sl.words);
    sstw_keep_kernel<<<unsigned(sstw::grid_for(cap)), sstw::kThreads, 0, s>>>(
        ok, reinterpret_cast<const unsigned long long*>(nblocks), status, cap, keep);
    KVSEP_HIP(hipGetLastError());
    // the salvage's layout and copy: a kept block's extent is its bytes and the 5-byte trailer that follows them
    r = launch_offsets_in(sc, s,
                          OffsetsCall{len, nullptr, keep, nullptr, 0, sstw::kTrailer, 0, ~uint64_t(0), dst_off,
                                      words + sstw::kDataEnd, nkept ? nkept : words + sstw::kSalvaged, cap, cap});
    if (r) return r;
    r = launch_pack<PackPlain>(c, s,
                               PackArgs{static_cast<const uint8_t*>(file_base), off,
                                        reinterpret_cast<const uint64_t*>(sc.off.p), nullptr,
                                        static_cast<uint8_t*>(dst), dst_bytes, dst_off, cap, cap, nullptr, nullptr, 0,
                                        0});
    if (r) return r;
    return launch_sst_build_in(c, sc, s, capturing,
                               SstBuildCall{file_base, key_off, key_len, dst_off, len, keep, cap, dst, dst_bytes,
                                            words + sstw::kDataEnd, index_len, wstatus, table_bytes, status});
  });
}

}  // extern "C"

namespace {
// ---- the chains pass and the records composite (crc32c_logchain.inc)

struct ChainCall {
  const uint8_t* type;
  const uint8_t* accept;
  const uint8_t* gap;
  const uint64_t* off;
  const uint64_t* len;
  const uint64_t* nrec;
  uint64_t cap;
  uint64_t* first;
  uint8_t* whole;
  uint64_t* frag_off;
  uint64_t* frag_len;
  uint64_t* nchain;
  uint64_t* nwhole;
};

// Refusals before any device is touched.
int chain_args(const char* who, const kvsep_crc32c_ctx* c, const ChainCall& k) {
  const bool any = k.off || k.len || k.frag_off || k.frag_len, all = k.off && k.len && k.frag_off && k.frag_len;
  const char* what = !c                                                           ? "null ctx"
                     : k.cap && (!k.type || !k.accept || !k.first || !k.whole)    ? "null type, accept, first or whole with cap != 0"
                     : any && !all                                                ? "off, len, frag_off and frag_len go together"
                     : !k.nrec                                                    ? "null nrec"
                     : !k.nchain                                                  ? "null nchain"
                     : k.cap > 0xffffffffull                                      ? "cap over 2^32 - 1"
                                                                                  : nullptr;
  if (!what) return KVSEP_OK;
  return set_err(KVSEP_EINVAL, (std::string(who) + ": " + what).c_str());
}

// The three kernels on `s`, on a scratch the caller has acquired and sized (ensure_chain).  cap == 0 runs the write
// kernel alone, which then touches no scratch.
int launch_chains_in(Scratch& sc, hipStream_t s, const ChainCall& k) {
  const uint64_t nt = chain::tile_count(k.cap);
  ChainArgs a{};
  a.type = k.type, a.accept = k.accept, a.gap = k.gap, a.off = k.off, a.len = k.len;
  a.nrec = reinterpret_cast<const unsigned long long*>(k.nrec);
  a.cap = k.cap, a.ntiles = nt;
  a.first = k.first, a.whole = k.whole, a.frag_off = k.frag_off, a.frag_len = k.frag_len;
  a.nchain = k.nchain, a.nwhole = k.nwhole;
  if (nt) {
    const chain::TileWords w = chain::tile_words(nt);
    a.sum = sc.chain.p + w.sum;
    a.in = sc.chain.p + w.in;
    a.grand = sc.chain.p + w.grand;
    chain_tile_kernel<<<unsigned(nt), chain::kThreads, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
    chain_scan_kernel<<<1, chain::kScanThreads, 0, s>>>(a.sum, a.in, a.grand, nt);
    KVSEP_HIP(hipGetLastError());
  }
  chain_write_kernel<<<unsigned(chain::write_tiles(k.cap)), chain::kThreads, 0, s>>>(a);
  KVSEP_HIP(hipGetLastError());
  return KVSEP_OK;
}
}  // namespace

extern "C" {

int kvsep_log_chains_device(kvsep_crc32c_ctx* c, void* stream, const uint8_t* type, const uint8_t* accept,
                            const uint8_t* gap, const uint64_t* off, const uint64_t* len, const uint64_t* nrec,
                            uint64_t cap, uint64_t* first, uint8_t* whole, uint64_t* frag_off, uint64_t* frag_len,
                            uint64_t* nchain, uint64_t* nwhole) {
  const ChainCall k{type, accept, gap, off, len, nrec, cap, first, whole, frag_off, frag_len, nchain, nwhole};
  int rc = chain_args("kvsep_log_chains_device", c, k);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_scratch(
      c, s, c->sc, [&](Scratch& sc, bool capturing) { return ensure_chain(sc, cap, capturing); },
      [&](Scratch& sc, bool) { return launch_chains_in(sc, s, k); });
}

int kvsep_log_records_device(kvsep_crc32c_ctx* c, void* stream, const void* base, uint64_t n, uint64_t* off,
                             uint64_t* len, uint32_t* stored, uint8_t* type, uint8_t* ok, uint8_t* accept, uint8_t* gap,
                             uint64_t cap, uint64_t* nrec, uint64_t* dropped, uint64_t* bad_length_bytes,
                             uint64_t* frag_off, uint64_t* frag_len, uint64_t* first, uint8_t* whole, uint64_t* nchain,
                             void* dst, uint64_t dst_bytes, uint64_t* rec_off, uint64_t* rec_len, uint64_t* end,
                             uint64_t* nwhole) {
  const char* who = "kvsep_log_records_device";
  const LogAcceptCall acc{base, n, off, len, type, ok, nrec, cap, accept, gap, dropped, bad_length_bytes};
  int rc = log_accept_args(who, c, acc);
  if (rc) return rc;
  if (cap && (!stored || !gap || !frag_off || !frag_len || !dst || !rec_off))
    return set_err(KVSEP_EINVAL, "kvsep_log_records_device: null stored, gap, frag_off, frag_len, dst or rec_off with cap != 0");
  if (!end) return set_err(KVSEP_EINVAL, "kvsep_log_records_device: null end");
  // the assembly state is read from gap[]: the fragment arrays are given whole, so the chains pass writes all four
  const ChainCall k{type, accept, gap, off, len, nrec, cap, first, whole, frag_off, frag_len, nchain, nullptr};
  rc = chain_args(who, c, k);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LogWalkCall w{base, n, off, len, stored, type, cap, nrec};
  const auto needs = [&](Scratch& sc, bool capturing) {  // the layout and the chains pass over cap chains, then the read
    int rc = ensure_offsets(sc, cap, capturing);
    if (!rc) rc = ensure_chain(sc, cap, capturing);
    if (!rc) rc = log_needs(c, n, true, cap)(sc, capturing);
    return rc;
  };
  return with_scratch(c, s, c->sc, needs, [&](Scratch& sc, bool capturing) {
    int r = launch_log_read_in(c, sc, s, capturing, w, acc, ok);
    if (!r) r = launch_chains_in(sc, s, k);
    // The layout: chain j is the fragments [first[j], first[j + 1]), kept when whole.  The walk's offsets pass is done
    // with the pass's scratch by now: its result went to the log words, which the fill kernel has read.
    if (!r)
      r = launch_offsets_in(sc, s, OffsetsCall{frag_len, first, whole, nullptr, 0, 0, 0, ~uint64_t(0), rec_off, end,
                                               nwhole, cap, cap});
    if (!r && rec_len && cap) {
      chain_reclen_kernel<<<unsigned(chain::reclen_grid(cap)), chain::kThreads, 0, s>>>(
          sc.off.p, rec_len, cap);
      if (hipGetLastError() != hipSuccess) r = set_err(KVSEP_EHIP, "chain_reclen_kernel launch");
    }
    if (!r)
      r = launch_pack<PackPlain>(c, s,
                                 PackArgs{static_cast<const uint8_t*>(base), frag_off, frag_len, first,
                                          static_cast<uint8_t*>(dst), dst_bytes, rec_off, cap, cap, nullptr, nullptr, 0,
                                          0});
    return r;
  });
}

// ---- the log / MANIFEST write side (crc32c_logframe.inc)
int kvsep_log_frame_device(kvsep_crc32c_ctx* c, void* stream, const void* base, const uint64_t* off,
                           const uint64_t* len, const uint8_t* keep, uint64_t count, uint64_t dest_length, void* dst,
                           uint64_t dst_bytes, uint64_t* rec_at, uint64_t* frag_first, uint64_t* frag_off,
                           uint64_t* frag_len, uint64_t* frag_at, uint8_t* frag_type, uint32_t* frag_crc,
                           uint64_t frag_cap, uint64_t* nfrag, uint64_t* written, uint64_t total_bytes) {
  const char* what =
      !c                                                                             ? "null ctx"
      : count && (!base || !off || !len || !rec_at)                                  ? "null base, off, len or rec_at with count != 0"
      : frag_cap && (!frag_off || !frag_len || !frag_at || !frag_type || !frag_crc || !dst)
          ? "null fragment array or dst with frag_cap != 0"
      : !frag_first || !nfrag || !written                                            ? "null frag_first, nfrag or written"
      : count > 0xffffffffull || frag_cap > 0xffffffffull                            ? "count or frag_cap over 2^32 - 1"
                                                                                     : nullptr;
  if (what) return set_err(KVSEP_EINVAL, (std::string("kvsep_log_frame_device: ") + what).c_str());
  // Value(&type, 1) for FULL .. LAST (log_writer.cc:16-21), once
  static const struct Seeds {
    uint32_t v[5];
    Seeds() {
      for (int t = 0; t < 5; ++t) {
        const char ch = char(t);
        v[t] = kvsep_crc32c_extend_host(0, &ch, 1);
      }
    }
  } seeds;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // every scratch size is checked before the first kernel: the two words of this pass, and the plan of the checksum
  // call when the context's piece size puts 32,761-byte fragments through one
  const auto needs = [&](Scratch& sc, bool capturing) {
    int rc = ensure_logw(sc, logw::fill_lanes(count, frag_cap), capturing);
    if (!rc && frag_cap) rc = ensure_plan_for(c, sc, frag_cap, total_bytes, logw::kAvail, capturing);
    return rc;
  };
  LogwArgs a{};
  a.off = off, a.len = len, a.keep = keep, a.count = count;
  a.b0 = logw::start_state(dest_length);
  a.dst = static_cast<uint8_t*>(dst), a.dst_bytes = dst_bytes;
  a.rec_at = rec_at, a.frag_first = frag_first;
  a.frag_off = frag_off, a.frag_len = frag_len, a.frag_at = frag_at, a.frag_type = frag_type, a.frag_cap = frag_cap;
  a.nfrag = nfrag, a.written = written;
  a.s1 = seeds.v[logw::kFull], a.s2 = seeds.v[logw::kFirst], a.s3 = seeds.v[logw::kMiddle], a.s4 = seeds.v[logw::kLast];
  return with_scratch(c, s, c->sc, needs, [&](Scratch& sc, bool capturing) -> int {
    a.rec = sc.logw.p, a.seed = sc.logw.q;
    logw_layout_kernel<<<1, logw::kLayoutThreads, 0, s>>>(a);
    KVSEP_HIP(hipGetLastError());
    const uint64_t lanes = logw::fill_lanes(count, frag_cap);
    if (lanes) {
      logw_fill_kernel<<<unsigned((lanes + logw::kFillThreads - 1) / logw::kFillThreads), logw::kFillThreads, 0, s>>>(a);
      KVSEP_HIP(hipGetLastError());
    }
    if (!frag_cap) return KVSEP_OK;
    // the fragments' checksums: the batched form over all frag_cap slots, the seeds as init (a padding slot has length
    // 0 and seed 0: frag_crc = 0 there), then the copy that stamps each header in front of its fragment
    int r = launch_batch_in(c, sc, s, capturing, base, frag_off, frag_len, sc.logw.q, nullptr, frag_crc, nullptr,
                            nullptr, frag_cap, total_bytes, logw::kAvail);
    if (r) return r;
    // fragment f is segment f: no first[]; a padding slot's kSkip lies in no destination (pack::fits)
    return launch_pack<PackLog>(c, s,
                                PackArgs{static_cast<const uint8_t*>(base), frag_off, frag_len, nullptr,
                                         static_cast<uint8_t*>(dst), dst_bytes, frag_at, frag_cap, frag_cap, frag_crc,
                                         frag_type, 0, 0});
  });
}

int kvsep_sst_verify_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, const uint64_t* off,
                            const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                            uint64_t total_bytes, uint64_t max_len) {
  if (!c || !file_base || !off || !len || !out) return set_err(KVSEP_EINVAL, "null argument");
  return sst_verify_device(c, stream, file_base, off, len, out, first_bad, nbad, count, total_bytes, max_len, nullptr);
}

int kvsep_sst_verify_list_device(kvsep_crc32c_ctx* c, void* stream, const void* file_base, const uint64_t* off,
                                 const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad,
                                 uint64_t* bad_idx, uint64_t bad_cap, uint8_t* ok, uint64_t count, uint64_t total_bytes,
                                 uint64_t max_len) {
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_device: null ctx");
  if (!bad_idx && bad_cap) return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_device: null bad_idx with bad_cap > 0");
  if (!file_base || !off || !len || !out) return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_device: null argument");
  const ListOut l{bad_idx, bad_cap, ok};
  return sst_verify_device(c, stream, file_base, off, len, out, first_bad, nbad, count, total_bytes, max_len, &l);
}

// The host-resident list form: the image and its handles go to the device for the call (blocking), the read check and
// its list pass run there, and the CRCs, the verdict and the list come back.
int kvsep_sst_verify_list_host(kvsep_crc32c_ctx* c, const char* file, uint64_t n, const uint64_t* off,
                               const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad,
                               uint64_t* bad_idx, uint64_t bad_cap, uint64_t count) {
  if (!c) return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_host: null ctx");
  if (!bad_idx && bad_cap) return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_host: null bad_idx with bad_cap > 0");
  if ((!file && n) || (count && (!off || !len || !out)))
    return set_err(KVSEP_EINVAL, "kvsep_sst_verify_list_host: null argument");
  uint64_t total = 0, max_len = 0;
  for (uint64_t i = 0; i < count; ++i) {
    // the handle must leave room for the 5-byte trailer (table/format.cc:84-87: "truncated block read")
    if (off[i] > n || len[i] > n - off[i] || n - off[i] - len[i] < 5)
      return set_err(KVSEP_EINVAL,
                     "kvsep_sst_verify_list_host: block handle (plus its 5-byte trailer) outside the file image");
    total += len[i];
    max_len = std::max(max_len, len[i]);
  }
  if (first_bad) *first_bad = ~0ull;
  if (nbad) *nbad = 0;
  if (!count) return KVSEP_OK;
  const uint64_t cap = std::min(bad_cap, count);
  struct Bufs {  // freed on every path
    void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Bufs() { for (void* q : p) hipFree(q); }
  } b;
  {
    DeviceGuard dg(c->device);
    KVSEP_HIP(dg.err);
    const size_t bytes[5] = {size_t(n), size_t(count * 16), size_t(count * 4), 16, size_t(std::max<uint64_t>(cap, 1) * 8)};
    for (int i = 0; i < 5; ++i)
      if (hipMalloc(&b.p[i], bytes[i]) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(KVSEP_ENOMEM, "kvsep_sst_verify_list_host: device allocation failed");
      }
    auto* d_off = static_cast<uint64_t*>(b.p[1]);
    auto* d_res = static_cast<uint64_t*>(b.p[3]);
    KVSEP_HIP(hipMemcpy(b.p[0], file, n, hipMemcpyHostToDevice));
    KVSEP_HIP(hipMemcpy(d_off, off, count * 8, hipMemcpyHostToDevice));
    KVSEP_HIP(hipMemcpy(d_off + count, len, count * 8, hipMemcpyHostToDevice));
    const int rc = kvsep_sst_verify_list_device(c, nullptr, b.p[0], d_off, d_off + count, static_cast<uint32_t*>(b.p[2]),
                                                d_res, d_res + 1, cap ? static_cast<uint64_t*>(b.p[4]) : nullptr, cap,
                                                nullptr, count, total, max_len);
    if (rc) return rc;
    uint64_t res[2];
    KVSEP_HIP(hipMemcpy(res, d_res, 16, hipMemcpyDeviceToHost));  // (the null stream: after the kernels)
    KVSEP_HIP(hipMemcpy(out, b.p[2], count * 4, hipMemcpyDeviceToHost));
    const uint64_t k = std::min(res[1], cap);
    if (k) KVSEP_HIP(hipMemcpy(bad_idx, b.p[4], k * 8, hipMemcpyDeviceToHost));
    if (first_bad) *first_bad = res[0];
    if (nbad) *nbad = res[1];
  }
  return KVSEP_OK;
}

const char* kvsep_crc32c_kernel_name(kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len) {
  if (!c) return "";
  std::lock_guard<std::mutex> g(c->mu);
  return route::kernel_name(route_of(c, count, total_bytes, max_len).form);
}

int kvsep_crc32c_plan_query(kvsep_crc32c_ctx* c, uint64_t count, uint64_t total_bytes, uint64_t max_len,
                            uint64_t* piece_bytes, uint64_t* pieces_needed, int* guided) {
  if (!c) return set_err(KVSEP_EINVAL, "null ctx");
  std::lock_guard<std::mutex> g(c->mu);
  const route::Route r = route_of(c, count, total_bytes, max_len);
  if (piece_bytes) *piece_bytes = r.piece.bytes;
  if (pieces_needed) *pieces_needed = r.pieces_needed;
  if (guided) *guided = r.dyn ? 1 : 0;
  return KVSEP_OK;
}

int kvsep_stream_read_device(kvsep_crc32c_ctx* c, void* stream, const void* src, uint64_t nbytes, uint32_t* sink) {
  if (!c || !src || !sink) return set_err(KVSEP_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t n16 = nbytes / 16;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device);
  KVSEP_HIP(dg.err);
  if (c->timing) {
    e0 = take_event(c);
    e1 = take_event(c);
    if (e0 && e1) KVSEP_HIP(hipEventRecord(e0, s));
  }
  if (!diag_stream_read(c, s, reinterpret_cast<uintptr_t>(src), n16, sink))  // KVSEP_DIAG build only
  stream_read_kernel<<<unsigned(c->num_cus), 512, 0, s>>>(reinterpret_cast<uintptr_t>(src), n16, sink);
  KVSEP_HIP(hipGetLastError());
  if (c->timing && e0 && e1) {
    KVSEP_HIP(hipEventRecord(e1, s));
    c->ev_pending.emplace_back(e0, e1);
  }
  return KVSEP_OK;
}

const char* kvsep_last_error(void) { return g_last_error.c_str(); }

}  // extern "C"
