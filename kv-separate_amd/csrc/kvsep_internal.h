// kvsep_internal.h -- declarations shared by the device (.hip) and host (.cpp) halves of
// libkvsep_crc32c.  Not part of the public ABI (include/kvsep_crc32c.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "copy_pool.h"

struct kvsep_crc32c_ctx;

namespace kvsep {

struct Scratch;

// One device array of a Scratch, or two that are sized together, with the capacity they hold -- in the unit the form
// that uses them counts in (blocks, tiles, records, lanes, restart runs), never bytes.  Nothing but these functions
// (crc32c_device.hip) allocates or frees a scratch array or sets a capacity; every array is a hipMalloc of its own.
// kEvenEmpty: the array exists even for a need of 0 (kernels that run on empty inputs write its stop word or totals).
constexpr bool kEvenEmpty = true;
template <typename T, bool kAlways = false, typename U = char>
struct __attribute__((visibility("hidden"))) DevBuf {  // (no symbol of it leaves the library)
  T* p = nullptr;
  U* q = nullptr;  // the second array of a pair (null where there is none)
  uint64_t cap = 0;
  bool holds(uint64_t need) const { return need <= cap && (p || !kAlways); }
  void drop();  // frees; cap = 0
  // np elements of p and nq of q, then cap = need; a failure leaves the buffer dropped
  int alloc(uint64_t need, uint64_t np, uint64_t nq = 0);
  // Room for `need`: nothing to do when it holds; under capture a refusal (KVSEP_EINVAL, `what`); else waits for the
  // scratch's last user (quiesce), drops and allocates -- a pair is freed whole before either array is allocated again.
  int ensure(Scratch& sc, uint64_t need, bool capturing, const char* what, uint64_t np, uint64_t nq = 0);
};

// Device scratch of one in-flight batch: the piece plan (planned mode), the work counter, the verify words and the
// arrays of the SST, list, offsets, log, chains, log-frame, SST-index and SST-build forms.  A scratch object is reused call after
// call; `last_use` orders a call on a different stream behind the previous user, so reuse across streams is race-free
// (crc32c_device.hip, with_scratch).  The host pipeline gives each staging slot its own Scratch so the two slots'
// batches overlap, and every graph capture takes a capture set's Scratch of its own (stream_scratch).
struct Scratch {
  DevBuf<uint64_t, false, uint64_t> plan_blocks;  // the plan: counts | pstart (one more), per block
  DevBuf<uint32_t, false, uint32_t> plan_pieces;  // ... and pblk | partial, per piece
  DevBuf<unsigned char> scan_tmp;                 // ... and hipcub's scan storage, in bytes
  DevBuf<uint32_t> counter;                       // the guided schedule's work counter
  DevBuf<unsigned long long> verify;  // [first_bad, nbad] when the caller passes none, then the accumulator set
  bool vacc_dirty = false;            // a failed eager call may have posted to the set: reset before its next use
  DevBuf<unsigned long long> vslot;   // captured verify calls: a verdict slot (2 words) per publishing workgroup
  DevBuf<uint64_t, false, uint32_t> sst;  // SST verify: len + 1 | the stored trailer words, per block
  // list forms: bad blocks per tile of the batch | their exclusive prefix sum (crc32c_verdicts.inc), per tile
  DevBuf<uint32_t, false, unsigned long long> tiles;
  // offsets pass (crc32c_offsets.inc): the extent of every block | offsets::scratch_words tile words, per block
  DevBuf<unsigned long long, false, unsigned long long> off;
  DevBuf<unsigned long long, kEvenEmpty> log;    // log reader (crc32c_logwalk.inc): logrun::scratch_words, per block
  DevBuf<unsigned long long, kEvenEmpty> chain;  // chains pass (crc32c_logchain.inc): chain::scratch_words, per record
  // log write side (crc32c_logframe.inc): a word per record | per fragment slot, per record / fragment slot
  DevBuf<uint32_t, kEvenEmpty, uint32_t> logw;
  DevBuf<unsigned long long, kEvenEmpty> sstidx;  // SST index walk (crc32c_sstindex.inc): sst::scratch_words, per run
  DevBuf<unsigned long long, kEvenEmpty> sstw;    // SST index build (crc32c_sstbuild.inc): sstw::scratch_words, per entry
  template <typename F>
  void each_buf(F f) {  // every array above: what free_scratch frees
    f(plan_blocks), f(plan_pieces), f(scan_tmp), f(counter), f(verify), f(vslot), f(sst), f(tiles), f(off), f(log),
        f(chain), f(logw), f(sstidx), f(sstw);
  }
  hipEvent_t last_use = nullptr;
  hipStream_t last_stream = nullptr;
  bool used = false;
};
void free_scratch(Scratch& sc);

// The persistent host copiers of the staging pipeline (copy_pool.h), bound to `cpus` when it is not empty.
CopyPool* copy_pool_create(const std::vector<int>& cpus);
void copy_pool_destroy(CopyPool* p);
void copy_pool_run(CopyPool* p, const CopySeg* segs, uint64_t nseg);  // returns when every byte is copied

// Double-buffered host<->device staging for the host-memory entry points.
struct HostStaging {
  static constexpr int kSlots = 2;
  uint64_t bytes = 0;        // payload bytes per slot
  uint64_t max_blocks = 0;   // descriptors per slot
  uint8_t* h_data[kSlots] = {nullptr, nullptr};   // pinned
  uint8_t* d_data[kSlots] = {nullptr, nullptr};
  uint64_t* h_desc[kSlots] = {nullptr, nullptr};  // pinned: off[max_blocks] | len[max_blocks]
  uint32_t* h_init[kSlots] = {nullptr, nullptr};  // pinned
  uint32_t* h_out[kSlots] = {nullptr, nullptr};   // pinned
  uint64_t* d_desc[kSlots] = {nullptr, nullptr};
  uint32_t* d_init[kSlots] = {nullptr, nullptr};
  uint32_t* d_out[kSlots] = {nullptr, nullptr};
  hipStream_t stream[kSlots] = {nullptr, nullptr};
  hipEvent_t done[kSlots] = {nullptr, nullptr};
  Scratch scratch[kSlots];
  CopyPool* pool = nullptr;
  std::vector<int> cpus;     // the CPUs the copiers (and the staging allocation) were bound to: the device's NUMA node
  bool ready = false;
  // allocation failed: retried only after a backoff (ensure_staging), so a transient failure is not permanent and
  // a persistent one does not cost an allocation attempt per call
  int64_t retry_at_ns = 0;
  uint32_t failures = 0;
};

void release_staging(HostStaging& s);

// Makes `dev` the calling thread's current HIP device for the scope and restores the caller's device on every
// exit path: the library never leaves a thread on another GPU than the one it came in with.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      prev = -1;
    }
    if (prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int now = -1;
    if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Implemented in crc32c_device.hip; callers hold ctx_mutex.
int device_batch_locked(kvsep_crc32c_ctx* c, Scratch& sc, hipStream_t s, const void* base, const uint64_t* off,
                        const uint64_t* len, const uint32_t* init, uint32_t* out, uint64_t count,
                        uint64_t total_bytes, uint64_t max_len);
// kvsep_crc32c_batch_host with an optional tee: tee[i] (when tee and tee[i] are non-null) also receives record i's bytes
// from the gather that stages them (crc32c_host.cpp).  Takes the context's mutex.
int batch_host_tee(kvsep_crc32c_ctx* c, const uint32_t* init, const char* const* ptr, const uint64_t* len,
                   uint32_t* out, uint64_t count, char* const* tee);
HostStaging& ctx_staging(kvsep_crc32c_ctx* c);
std::mutex& ctx_mutex(kvsep_crc32c_ctx* c);
int ctx_device(kvsep_crc32c_ctx* c);
int ctx_host_node(kvsep_crc32c_ctx* c);  // NUMA node of the device (-1: unknown or binding off)
uint64_t ctx_piece_bytes(kvsep_crc32c_ctx* c);
void set_last_error(const char* msg);

}  // namespace kvsep
