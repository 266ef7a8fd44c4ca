/*
 * kvsep_crc32c.h -- C ABI of the MI355X-native CRC-32C-over-blocks engine (libkvsep_crc32c.so).
 *
 * Drop-in boundary for the checksum hot path of Buildings-Lei/kv-separate:
 *   util/crc32c.h:17   uint32_t leveldb::crc32c::Extend(uint32_t init_crc, const char* data, size_t n)
 *   util/crc32c.h:20   Value(data, n) = Extend(0, data, n)
 *   util/crc32c.h:22-38 kMaskDelta / Mask / Unmask
 *   port/port_stdcxx.h:142-152  port::AcceleratedCRC32C(crc, buf, size)  -- the reference's own
 *                      plug point for an accelerated backend (self-test util/crc32c.cc:267-274)
 * plus batched entry points that the reference's call sites would bind to when they hold a batch
 * of independent records/blocks:
 *   db/value_log_reader.cc:86-138  vlog record verify (recovery db/db_impl.cc:485-571, GC :880-951)
 *   db/value_log_writer.cc:46-76   vlog record checksum before Append
 *   table/table_builder.cc:209-232, table/format.cc:99-108  SST block trailers
 *   db/log_writer.cc:84-115, db/log_reader.cc:246-259  MANIFEST fragments (per-type init CRC)
 *
 * All pointers are plain; no framework types cross this boundary.  Results are bit-exact with
 * util/crc32c.cc (checked by tests/ against golden vectors captured from the compiled reference).
 */
#ifndef KVSEP_CRC32C_H_
#define KVSEP_CRC32C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  2 (round 3): kvsep_vlog_verify_host takes *drop_bytes (7 arguments) and kvsep_crc32c_kernel_name
 * takes total_bytes before max_len -- both changed in place from ABI 1, so a caller built against ABI 1 must be
 * rebuilt; check kvsep_abi_version() == KVSEP_ABI_VERSION once at startup.  3 (round 5): kvsep_offload_stats counts
 * only calls at or above the offload threshold (since round 4: host_calls no longer includes the calls below it, which
 * are not counted at all); new entry points for the host legs, topology and host placement; no signature changed.
 * 4 (round 6): graph captures get capture sets of their own (kvsep_crc32c_reserve_captures / _release_captures /
 * _capture_sets); the fault-injection hook left this header (csrc/kvsep_testing.h) and works only under
 * KVSEP_TEST_HOOKS=1; no signature changed.  ABI 4 later gained the list forms of the verify calls
 * (kvsep_crc32c_verify_list_device, kvsep_sst_verify_list_device / _host, kvsep_log_verify_device,
 * kvsep_crc32c_group_verify_list_device): new entry points only, no signature changed, so the version stays 4; the
 * combine, concat and gather forms (kvsep_crc32c_combine, kvsep_crc32c_concat_device, kvsep_crc32c_gather_device /
 * _host, kvsep_crc32c_group_extend_host) came the same way, and so did the device write side
 * (kvsep_crc32c_pack_device, kvsep_vlog_frame_offsets, kvsep_vlog_frame_device, kvsep_sst_frame_device) and the
 * offsets and salvage forms (kvsep_crc32c_offsets_device, kvsep_crc32c_salvage_device, kvsep_sst_salvage_device,
 * kvsep_vlog_frame_auto_device) and the device log / MANIFEST reader (kvsep_log_walk_device,
 * kvsep_log_accept_gaps_device, kvsep_log_read_device) and its record assembly (kvsep_log_chains,
 * kvsep_log_chains_device, kvsep_log_records_device) and the device log / MANIFEST writer (kvsep_log_frame_layout,
 * kvsep_log_frame_device) and the SST table reader (kvsep_sst_footer, kvsep_sst_index_walk, kvsep_sst_index_device,
 * kvsep_sst_table_verify_device, the KVSEP_SST_* status codes) and the SST table writer (kvsep_sst_index_keys,
 * kvsep_sst_index_keys_device, kvsep_sst_index_build, kvsep_sst_footer_build, kvsep_sst_index_build_device,
 * kvsep_sst_table_finish_device, kvsep_sst_table_rewrite_device, KVSEP_SST_SHARED_KEY, the KVSEP_SSTW_* status codes)
 * and the device value-log reader (kvsep_vlog_walk_device, kvsep_vlog_read_device).
 * The reference's C++ symbol leveldb::crc32c::Extend is not in this library: it is in the libkvsep_leveldb_abi.so
 * shim. */
#define KVSEP_ABI_VERSION 4
int kvsep_abi_version(void);

#define KVSEP_OK 0
#define KVSEP_EINVAL (-1)  /* bad argument */
#define KVSEP_EHIP (-2)    /* a HIP runtime call failed (message via kvsep_last_error) */
#define KVSEP_ENODEV (-3)  /* no usable gfx950 device */
#define KVSEP_ENOMEM (-4)  /* device or pinned allocation failed */

/* ---------------------------------------------------------------- scalar drop-in
 * Same contract as util/crc32c.h:17 / util/crc32c.cc:276: CRC-32C of A||data[0,n) where
 * init_crc = crc32c(A); n == 0 returns init_crc; any alignment; never fails; reentrant.
 * Dispatch: n >= the offload threshold (kvsep_set_offload_threshold, default 64 MiB) goes through
 * the GPU (pinned staging, H2D, kernel, D2H); smaller inputs use the host leg (VPCLMULQDQ folding on CPUs with
 * AVX-512 carry-less multiply, else SSE4.2 crc32 -- the role google/crc32c plays behind port::AcceleratedCRC32C). */
uint32_t kvsep_crc32c_extend(uint32_t init_crc, const char* data, size_t n);
uint32_t kvsep_crc32c_value(const char* data, size_t n); /* util/crc32c.h:20 */
uint32_t kvsep_crc32c_mask(uint32_t crc);                /* util/crc32c.h:29-32 */
uint32_t kvsep_crc32c_unmask(uint32_t masked_crc);       /* util/crc32c.h:35-38 */
/* port/port_stdcxx.h:142: returns Extend(crc, buf, size); never 0 for the self-test buffer. */
uint32_t kvsep_accelerated_crc32c(uint32_t crc, const char* buf, size_t size);
void kvsep_set_offload_threshold(uint64_t nbytes);
/* A call at/above the threshold while another caller holds the device's GPU leg: wait != 0 queues it for the
 * GPU; wait == 0 (the default) runs it on the host leg at once -- the reference calls Extend from the writer,
 * compaction, GC and reader threads concurrently (db/db_impl.cc:1829-1833), and one PCIe link serves one
 * staged copy at a time while every core can run the host leg. */
void kvsep_set_offload_wait(int wait);
/* Counters of the scalar drop-in's calls at/above the offload threshold since load (any may be null): calls
 * served by the GPU, calls diverted to the host leg because the GPU leg was busy, and calls that the GPU could
 * not serve and that finished on the host (set KVSEP_STRICT_GPU=1 to abort on those instead).  Calls below the
 * threshold are not counted (no shared counter on the small-call path). */
void kvsep_offload_stats(uint64_t* gpu_calls, uint64_t* host_calls, uint64_t* gpu_failures);
/* Host-only CRC, the small-input leg of Extend, on the fastest leg this CPU runs (checked once, at first use):
 * "fold" (x86-64 with AVX-512F + VPCLMULQDQ: 4 x 512-bit accumulators), else "sse42" (x86-64 with SSE4.2: the crc32
 * instruction, 3-way interleaved), else "portable" (any CPU: table-driven, slicing-by-8).  KVSEP_HOST_CRC=sse42 or
 * =portable forces a slower leg.  Exact on every leg; never an illegal instruction on a CPU without the extension. */
uint32_t kvsep_crc32c_extend_host(uint32_t init_crc, const char* data, size_t n);
/* The leg kvsep_crc32c_extend_host runs in this process: "fold", "sse42" or "portable". */
const char* kvsep_crc32c_host_path(void);

/* ---------------------------------------------------------------- device context */
typedef struct kvsep_crc32c_ctx kvsep_crc32c_ctx;

int kvsep_crc32c_ctx_create(int device, kvsep_crc32c_ctx** out);
void kvsep_crc32c_ctx_destroy(kvsep_crc32c_ctx* ctx);
/* Work-item ("piece") size for splitting long blocks; default 128 KiB, min 1 KiB, multiple of 1 KiB. */
int kvsep_crc32c_ctx_set_piece_bytes(kvsep_crc32c_ctx* ctx, uint64_t piece_bytes);
/* 0 = static contiguous runs of work items per wave, 2 = static round-robin items, 1 = guided dynamic (one atomic
 * per run of items), -1 = auto (default): guided when long blocks are split into pieces, else static. */
int kvsep_crc32c_ctx_set_schedule(kvsep_crc32c_ctx* ctx, int dynamic);
/* Kernel of unsplit batches: 0 = auto (default; the narrow kernel for many blocks <= 8-32 KiB, its sorted-window
 * form when the batch is ragged: max_len > 1.25 x total_bytes / count), 1 = always the wide kernel, 2 = the narrow
 * kernel whenever max_len <= 64 KiB, 3 / 4 = as 2 with 16- / 8-wave workgroups, 5 = as 2 in the sorted-window form,
 * 6 = as 2 with each workgroup's contiguous run of groups dealt to its waves by an LDS claim counter (round 4; auto
 * takes it for uniform batches of 32 Ki - 384 Ki blocks <= 4 KiB, 32 Ki - 64 Ki blocks of 4-8 KiB), 7 = as 6 with
 * 16 lanes per block, 4-block groups (auto: uniform batches of >= 4 Ki blocks of 8-12 KiB, up to 512 MiB), 8 = the
 * narrow kernel whose workgroup's 8 waves share each 8-block group (round 6; blocks over 4 KiB take its wide path;
 * auto never picks it: 1.5x the claim kernel's time on 4 KiB blocks).
 * A choice of speed only: every kernel is exact for every block.  No environment variable changes it. */
int kvsep_crc32c_ctx_set_kernel(kvsep_crc32c_ctx* ctx, int kernel);
/* NUMA node the context's host legs are placed on: its pinned staging is allocated, and its copier threads run, on
 * the CPUs of this node that the allocating thread may use.  Default: the node of the device's PCI function
 * (kvsep_device_numa_node); -1 = no placement.  Takes effect for staging not yet allocated (set it before the first
 * host-form call).  The group forms also bind each member's host thread to its member's node for the call. */
int kvsep_crc32c_ctx_set_host_node(kvsep_crc32c_ctx* ctx, int node);
/* Where the context's host legs are: *device_node = the node it places them on (-1: none), *staging_node = the node
 * holding its first pinned staging slot (-1: not allocated yet / unknown), cpus[0..cap) = the CPUs its copier threads
 * are bound to.  Returns the number of those CPUs (0: not bound), or KVSEP_EINVAL. */
int kvsep_crc32c_ctx_host_placement(kvsep_crc32c_ctx* ctx, int* device_node, int* staging_node, int* cpus, int cap);
/* Pre-size scratch so later calls of up to `count` blocks / `total_bytes` bytes do not allocate: the context's own
 * scratch (eager calls) and every free capture set (at least 4 are made).  Required before graph capture; covers the
 * planned, narrow, verify, list, SST-verify, offsets, salvage, log-read and record-assembly forms: any batch within both numbers, whatever piece size it picks, and the SST
 * read check called with the caller's own total_bytes. */
int kvsep_crc32c_reserve(kvsep_crc32c_ctx* ctx, uint64_t count, uint64_t total_bytes);
/* Graph capture (hipStreamBeginCapture ... EndCapture, torch.cuda.graph): every call captured into one graph runs on
 * that capture's own capture set -- its piece plan, work counter, SST arrays and verify verdict slots -- held by it until
 * kvsep_crc32c_release_captures.  So graphs of one context may be replayed at the same time on different streams, and
 * a verify graph replayed over itself (two streams, two instantiations) writes identical verdicts.  The calls of ONE
 * graph share its set and must be ordered inside the graph (captured on one stream, or joined); a graph holding
 * planned batches (max_len 0 or above the piece size) must not overlap a replay of itself.  A capture that finds no free
 * set fails with KVSEP_EINVAL when its first call is captured.
 * reserve_captures: at least nsets sets, free ones sized by the largest kvsep_crc32c_reserve so far (held sets keep the
 *   size their graph captured).
 * release_captures: every set free again -- call it only once the graphs captured so far are destroyed (a later
 *   reserve may reallocate a free set).
 * capture_sets: returns the number of sets; *held (nullable) = how many a graph holds. */
int kvsep_crc32c_reserve_captures(kvsep_crc32c_ctx* ctx, int nsets);
int kvsep_crc32c_release_captures(kvsep_crc32c_ctx* ctx);
int kvsep_crc32c_capture_sets(kvsep_crc32c_ctx* ctx, int* held);
/* Kernel timing with HIP events on the caller's stream, around the main CRC kernel only. */
int kvsep_crc32c_ctx_set_timing(kvsep_crc32c_ctx* ctx, int enable);
int kvsep_crc32c_ctx_get_timing(kvsep_crc32c_ctx* ctx, double* total_ms, uint64_t* launches); /* syncs + resets */
/* Name of the main kernel a batch of `count` blocks with these total_bytes / max_len hints runs on
 * ("crc32c_pieces_kernel", "crc32c_narrow_kernel", "crc32c_narrow_claim_kernel" or "crc32c_narrow_sorted_kernel"):
 * the kernel the timing above
 * and a rocprofv3 trace refer to. */
const char* kvsep_crc32c_kernel_name(kvsep_crc32c_ctx* ctx, uint64_t count, uint64_t total_bytes, uint64_t max_len);

/* ---------------------------------------------------------------- batched device form
 * out[i] = Extend(init ? init[i] : 0, base + off[i], len[i]) for i < count.
 * base/off/len/init/out are DEVICE pointers; the call is asynchronous on `stream`
 * (a hipStream_t; NULL = default stream).  Blocks may overlap and sit at any byte alignment.
 * total_bytes ~ sum(len) and max_len (an upper bound on len[i], or 0 if unknown) are performance hints:
 * with max_len <= piece size (128 KiB) the planning pass is skipped and short blocks may run on the narrow
 * kernel.  Results are exact whatever the hints say: a block longer than max_len is checksummed whole by
 * the wide kernel or deferred by the narrow one, and an understated total_bytes makes the kernel fall back
 * to one work item per block.  count <= 2^32 - 1, and <= 2^31 - 1 when the batch is planned (max_len 0 or
 * above the piece size); else KVSEP_EINVAL.
 * Memory touched (this form and the verify form below): the payload needs no padding -- a block may start on the
 * first byte of a mapping and end on its last.  The kernels read only naturally aligned 16-B granules that hold at
 * least one byte of a block of the batch (the cooperative kernel, reachable through kvsep_crc32c_ctx_set_kernel
 * only: 128-B lines that do), so never a page no block touches.  A block with len[i] == 0 is never dereferenced,
 * whatever off[i] is; out[i] = its init.  off, len, init (and expected_masked) are read for exactly `count`
 * elements, out is written for exactly `count`; the payload is never written.  The list forms write bad_idx for at
 * most bad_cap elements (exactly min(*nbad, bad_cap), the rest is left as it was) and ok for exactly `count`. */
int kvsep_crc32c_batch_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                              const uint64_t* len, const uint32_t* init, uint32_t* out, uint64_t count,
                              uint64_t total_bytes, uint64_t max_len);

/* Verify form: as above, plus Mask(out[i]) is compared with expected_masked[i] (the stored LE32
 * header word of db/value_log_writer.cc:58-59).  *first_bad (device) receives the lowest mismatching
 * index or UINT64_MAX, *nbad the number of mismatches -- the reader truncates at the first bad
 * record (db/value_log_reader.cc:112-122), so callers keep records [0, *first_bad). */
int kvsep_crc32c_verify_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                               const uint64_t* len, const uint32_t* init, const uint32_t* expected_masked,
                               uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                               uint64_t total_bytes, uint64_t max_len);

/* List form: kvsep_crc32c_verify_device, followed on the same stream by a device pass that says WHICH blocks
 * mismatch -- what a reader that skips exactly the bad blocks and keeps the rest needs (RepairDB::ScanTable,
 * db/repair.cc:220-260; paranoid reads, table/format.cc:99-106), where *first_bad / *nbad serve a reader that truncates.
 *   bad_idx[0 .. min(*nbad, bad_cap))  (device, u64) the mismatching block indices, ascending.  Nothing is written past
 *                                      that; *nbad is the full count, so *nbad > bad_cap says the list was cut.
 *                                      May be NULL iff bad_cap == 0.
 *   ok[0 .. count)                     (device, u8, nullable) 1 where Mask(out[i]) == expected_masked[i], else 0; every
 *                                      byte is written, on a clean batch too.
 * first_bad / nbad may be NULL as in the verify form.  On a clean batch with ok == NULL the list pass costs its three
 * launches only: each returns after loading *nbad.  Scratch (one word and one base per 1,024 blocks) is sized by
 * kvsep_crc32c_reserve(ctx, count, ...) like the other forms', so a reserved call allocates nothing and can be
 * captured; a captured call with more blocks than reserved fails with KVSEP_EINVAL. */
int kvsep_crc32c_verify_list_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                                    const uint64_t* len, const uint32_t* init, const uint32_t* expected_masked,
                                    uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t* bad_idx,
                                    uint64_t bad_cap, uint8_t* ok, uint64_t count, uint64_t total_bytes,
                                    uint64_t max_len);

/* ---------------------------------------------------------------- combine, concat and gather forms
 * Value(X) = Extend(0, X).  For every byte string B and every c, Extend(c, B) = c * x^(8|B|) ^ Value(B) (products mod
 * the CRC polynomial; Extend's pre- and post-inversion cancel), so the CRC of A||B follows from the CRCs of its parts
 * -- what zlib's crc32_combine and RocksDB's Crc32cCombine give.  ABI 4 gained these as new entry points only. */
/* Returns Extend(crc_a, B) for crc_b = Value(B), len_b = |B|: Value(A||B) when crc_a = Value(A).  Host only, pure,
 * never fails, needs no device; exact for every len_b up to 2^64 - 1; len_b == 0 returns crc_a. */
uint32_t kvsep_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* Batched combine on the device.  Block i is the run of segments j in [first[i], first[i + 1]), in order, and
 *   out[i] = fold over the run of  acc = kvsep_crc32c_combine(acc, seg_crc[j], seg_len[j]),  acc = init ? init[i] : 0
 * = Extend(init[i], the segments' bytes back to back) when seg_crc[j] = Value(segment j).  A block with no segments
 * gives its init; a segment of length 0 leaves acc as it is.  Only CRCs and lengths are read, never payload: seg_len[j]
 * may be anything up to 2^64 - 1.  All arrays are DEVICE pointers; asynchronous on `stream`; one kernel launch, no
 * library scratch, no atomics, no verdict: needs no kvsep_crc32c_reserve and can be captured as it is.
 * count <= 2^32 - 1, else KVSEP_EINVAL.
 * Memory touched: first is read for exactly count + 1 elements and out is written for exactly count.  Every first[]
 * value is clamped to nseg before use and a run that ends before it starts is empty, so seg_crc / seg_len are read at
 * indices < nseg only, whatever first[] holds (with nseg == 0 they may be NULL); init is read for exactly count. */
int kvsep_crc32c_concat_device(kvsep_crc32c_ctx* ctx, void* stream, const uint32_t* seg_crc, const uint64_t* seg_len,
                               const uint64_t* first, const uint32_t* init, uint32_t* out, uint64_t count,
                               uint64_t nseg);

/* Gather (iovec) form: block i is the concatenation, in order, of the segments [base + seg_off[j], + seg_len[j]) for
 * j in [first[i], first[i + 1]), which may lie anywhere -- out of order, overlapping, shared between blocks -- and
 *   out[i] = Extend(init ? init[i] : 0, that concatenation),
 * without the block being copied together first (a group-commit batch still lying as its members, a record as its
 * FIRST / MIDDLE / LAST fragments).  It is kvsep_crc32c_batch_device over the nseg segments with no init, writing
 * seg_crc[j] = Value(segment j) (the caller's array of nseg words, useful in its own right), followed on the same
 * stream by kvsep_crc32c_concat_device.  total_bytes / max_len are the hints of kvsep_crc32c_batch_device applied to
 * the segments, with its limits (nseg <= 2^32 - 1; 2^31 - 1 when planned); every route serves the segment pass.
 * kvsep_crc32c_reserve(ctx, nseg, total_bytes) makes the call allocation-free and capturable.
 * Memory touched: as kvsep_crc32c_batch_device for base / seg_off / seg_len over nseg segments (a segment of length 0
 * is never dereferenced); seg_crc is written for exactly nseg elements; first, init and out as in
 * kvsep_crc32c_concat_device; the payload and the descriptor arrays are never written. */
int kvsep_crc32c_gather_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* seg_off,
                               const uint64_t* seg_len, const uint64_t* first, const uint32_t* init, uint32_t* seg_crc,
                               uint32_t* out, uint64_t count, uint64_t nseg, uint64_t total_bytes, uint64_t max_len);
/* Host-pointer gather form: segment j is [seg_ptr[j], + seg_len[j]) in host memory.  kvsep_crc32c_batch_host over the
 * segments (pinned staging, as the batched host form), then the same fold on the host; blocking.  first[] is clamped
 * as in the device form; a segment of length 0 is never dereferenced. */
int kvsep_crc32c_gather_host(kvsep_crc32c_ctx* ctx, const uint32_t* init, const char* const* seg_ptr,
                             const uint64_t* seg_len, const uint64_t* first, uint32_t* out, uint64_t count,
                             uint64_t nseg);

/* ---------------------------------------------------------------- pack and frame forms (device write side)
 * The CRC forms above checksum a block as its segments lie; these move its bytes, so that a batch resident on the
 * device becomes the image the reference's writers would produce, ready for one pwrite.  ABI 4 gained them as new entry
 * points only. */
/* Batched gather-copy: block i is the segments j in [first[i], first[i + 1]), in order, each [base + seg_off[j],
 * + seg_len[j]); their bytes go back to back to dst + dst_off[i].  Segments may lie anywhere -- out of order,
 * overlapping, shared between blocks.  All arrays are DEVICE pointers; asynchronous on `stream`; one kernel launch
 * (crc32c_pack_kernel), no library scratch, no atomics, no verdict: needs no kvsep_crc32c_reserve and can be captured as
 * it is.  count <= 2^32 - 1, else KVSEP_EINVAL; a null ctx, or a null first / dst / dst_off with count != 0, or a null
 * seg_off / seg_len with nseg != 0, is KVSEP_EINVAL before any device is touched.
 * Memory touched.  Writes are byte-exact: block i writes [dst + dst_off[i], + len_i), len_i = the sum of its run's
 * seg_len, and no other byte -- no edge is written through a wider word, so blocks may sit back to back at any
 * alignment.  A block that does not lie wholly inside [0, dst_bytes) (its length may leave 64 bits) is not written at
 * all.  Reads stay inside the naturally aligned 16-B granules that hold a byte of a segment of the batch; a segment of
 * length 0 is never dereferenced.  first is read for exactly count + 1 elements, every value clamped to nseg and a run
 * that ends before it starts empty, as in kvsep_crc32c_concat_device; dst_off for exactly count; seg_off / seg_len at
 * indices < nseg only (with nseg == 0 they may be NULL).  The destination ranges of different blocks must not overlap
 * each other or any segment: where they do, the bytes written are unspecified (the ranges written are not). */
int kvsep_crc32c_pack_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* seg_off,
                             const uint64_t* seg_len, const uint64_t* first, void* dst, uint64_t dst_bytes,
                             const uint64_t* dst_off, uint64_t count, uint64_t nseg);
/* Offsets of vlog records laid back to back from `start`: rec_off[i] = start + sum over k < i of (8 + len[k]), *end
 * (nullable) = start + the sum over all.  Host arrays, pure, no device.  KVSEP_EINVAL for a len over 2^32 - 1 (the
 * header's LE32 length, db/value_log_writer.cc:48) or a sum that leaves 64 bits. */
int kvsep_vlog_frame_offsets(const uint64_t* len, uint64_t count, uint64_t start, uint64_t* rec_off, uint64_t* end);
/* vlog write side for device-resident members (VlogWriter::AddRecord, db/value_log_writer.cc:46-76): record i's payload
 * is the segments [first[i], first[i + 1]) as in kvsep_crc32c_gather_device.  It is that call without init (seg_crc[j]
 * = Value(segment j) for nseg words, crc_out[i] = Value(payload i) for count words), followed on the same stream by the
 * gather-copy above, which also writes the header: dst + rec_off[i] holds [Mask(crc_out[i]) LE32][len_i LE32][payload].
 * rec_off comes from kvsep_vlog_frame_offsets or the caller's own prefix sum.  The length word is the low 32 bits of
 * len_i: a payload of 2^32 bytes or more is the caller's error.  total_bytes / max_len are the hints of the CRC pass
 * over the segments, with its limits; kvsep_crc32c_reserve(ctx, nseg, total_bytes) makes the call allocation-free and
 * capturable.  Memory touched: as the two calls; a record that does not lie inside [0, dst_bytes) is not written. */
int kvsep_vlog_frame_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* seg_off,
                            const uint64_t* seg_len, const uint64_t* first, uint32_t* seg_crc, uint32_t* crc_out,
                            void* dst, uint64_t dst_bytes, const uint64_t* rec_off, uint64_t count, uint64_t nseg,
                            uint64_t total_bytes, uint64_t max_len);
/* SST write side for device-resident blocks (TableBuilder::WriteRawBlock, table/table_builder.cc:209-232):
 * kvsep_sst_trailers_device (masked_out[i] for count words), followed on the same stream by the gather-copy with block
 * i = [base + off[i], + len[i]): dst + blk_off[i] holds [block][types[i]][masked_out[i] LE32], the bytes a handle
 * (blk_off[i], len[i]) reads back.  Hints, limits and reserve(ctx, count, total_bytes) as kvsep_sst_trailers_device;
 * types and masked_out are required, off / len / dst / blk_off when count != 0. */
int kvsep_sst_frame_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                           const uint64_t* len, const uint8_t* types, uint32_t* masked_out, void* dst,
                           uint64_t dst_bytes, const uint64_t* blk_off, uint64_t count, uint64_t total_bytes,
                           uint64_t max_len);

/* ---------------------------------------------------------------- offsets and salvage forms (layout on the device)
 * The pack and frame forms above take their destination offsets from the caller.  These compute them on the device
 * from a verdict that is on the device, so that check -> choose -> lay out -> copy runs on one stream with no host step
 * and can be captured.  ABI 4 gained them as new entry points only. */
#define KVSEP_OFFSET_SKIP UINT64_MAX /* dst_off of a block that is not laid out */
/* Masked offset scan.  Block i is the segments j in [first[i], first[i + 1]) of seg_len (first == NULL: block i is
 * segment i), size_i the sum of their lengths.  The kept blocks are laid back to back from `start`, each taking
 * head_bytes + size_i + tail_bytes:
 *   dst_off[i] = start + the sum over kept k < i of (head_bytes + size_k + tail_bytes)   for a kept block,
 *   dst_off[i] = KVSEP_OFFSET_SKIP                                                       for a dropped one,
 *   *end       = start + the sum over every kept block,   *nkept (nullable) = the number of kept blocks.
 * The keep rule is one of: keep[i] != 0 (a device u8 array: the ok[] of the list forms); i < *keep_before (a device u64:
 * the *first_bad of a verify call, UINT64_MAX keeps all); neither: every block.  Passing both is KVSEP_EINVAL.
 * Every sum saturates at 2^64 - 1: a kept block whose end reaches that value gets KVSEP_OFFSET_SKIP, and so does every
 * kept block after it; *end is then UINT64_MAX (*nkept still counts them).  The pack forms write no block at
 * KVSEP_OFFSET_SKIP (it lies inside no destination), so dst_off can be handed to them as it is.
 * All arrays are DEVICE pointers; asynchronous on `stream`; three small kernels ordered by the stream (no atomics), on
 * library scratch of 8 bytes per block sized by kvsep_crc32c_reserve(ctx, count, ...): a reserved call allocates nothing
 * and can be captured; a captured call with more blocks than reserved fails with KVSEP_EINVAL before anything is
 * enqueued.  count <= 2^32 - 1, else KVSEP_EINVAL.  The argument refusals come before any device is touched.
 * Memory touched: first is read for exactly count + 1 elements, every value clamped to nseg and a run that ends before
 * it starts empty, so seg_len is read at indices < nseg only (and only for kept blocks); keep for exactly count;
 * *keep_before is read; dst_off is written for exactly count, *end and *nkept once. */
int kvsep_crc32c_offsets_device(kvsep_crc32c_ctx* ctx, void* stream, const uint64_t* seg_len, const uint64_t* first,
                                const uint8_t* keep, const uint64_t* keep_before, uint64_t head_bytes,
                                uint64_t tail_bytes, uint64_t start, uint64_t* dst_off, uint64_t* end, uint64_t* nkept,
                                uint64_t count, uint64_t nseg);
/* Salvage copy: the kept blocks [base + off[i], + len[i]) go back to back to dst from offset 0.  It is the offsets pass
 * above (block i = segment i, head = tail = 0, start = 0; the same keep rules), followed on the same stream by
 * kvsep_crc32c_pack_device with the dst_off it wrote.  With keep_before = the first_bad of a verify call this is what
 * VlogReader returns (db/value_log_reader.cc:109-122): everything before the first bad record.  dst_off (count words),
 * *end and *nkept are outputs; a kept block that does not lie inside [0, dst_bytes) is not written (*end says what
 * was needed); no byte of dst past *end is written. */
int kvsep_crc32c_salvage_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                                const uint64_t* len, const uint8_t* keep, const uint64_t* keep_before, void* dst,
                                uint64_t dst_bytes, uint64_t* dst_off, uint64_t* end, uint64_t* nkept, uint64_t count);
/* SST salvage (RepairDB::ScanTable, db/repair.cc:220-260; paranoid compaction inputs): kvsep_sst_verify_list_device
 * with ok[] (required; out, first_bad, nbad as there), then the offsets pass with keep = ok and tail = 5, then the
 * gather-copy of len[i] + 5 bytes per passed block: dst holds the passed blocks with their trailers, contiguous from 0,
 * dst_off[i] where block i went (a handle (dst_off[i], len[i]) reads it back), *end the bytes used.  Hints, limits and
 * reserve(ctx, count, total_bytes) as kvsep_sst_verify_list_device. */
int kvsep_sst_salvage_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, const uint64_t* off,
                             const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint8_t* ok,
                             void* dst, uint64_t dst_bytes, uint64_t* dst_off, uint64_t* end, uint64_t* nkept,
                             uint64_t count, uint64_t total_bytes, uint64_t max_len);
/* kvsep_vlog_frame_device with the record offsets computed on the device: the gather pass, the offsets pass (head = 8,
 * every record kept, from `start`) writing rec_off (count words, an output here) and *end, then the Vlog gather-copy.
 * A payload over 2^32 - 1 bytes, which kvsep_vlog_frame_offsets refuses, gets KVSEP_OFFSET_SKIP, as does every record
 * after it, and *end = UINT64_MAX: none of them is written.  reserve(ctx, max(count, nseg), total_bytes) makes the call
 * allocation-free and capturable. */
int kvsep_vlog_frame_auto_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* seg_off,
                                 const uint64_t* seg_len, const uint64_t* first, uint32_t* seg_crc, uint32_t* crc_out,
                                 void* dst, uint64_t dst_bytes, uint64_t start, uint64_t* rec_off, uint64_t* end,
                                 uint64_t count, uint64_t nseg, uint64_t total_bytes, uint64_t max_len);

/* ---------------------------------------------------------------- log / MANIFEST reader on the device
 * kvsep_log_walk and kvsep_log_accept_gaps for a log image that is on the device, so that walk -> checksum -> verdict
 * runs on one stream with no host step and can be captured.  The format is cut into 32 KiB blocks and no physical
 * record spans two, so a lane walks a block; the record indices come from the offsets pass over the blocks' counts.
 * ABI 4 gained them as new entry points only.
 * Every array is a DEVICE pointer; every call is asynchronous on `stream`; results are identical from run to run (no
 * atomics).  The argument refusals come before any device is touched: a null ctx, a null base with n != 0, a null
 * required output with cap != 0, a null nrec, cap > 2^32 - 1 -- each KVSEP_EINVAL.
 * Scratch: a few words per 32 KiB block plus the offsets pass's, sized by kvsep_crc32c_reserve(ctx, count, total_bytes)
 * with count >= max(cap, ceil(n / 32768)) and total_bytes >= n: a reserved call allocates nothing and can be captured; a
 * captured call larger than the reservation fails with KVSEP_EINVAL before anything is enqueued.
 * Memory touched: the image is never written; it is read bytewise at header positions, so every read lies inside
 * [base, base + n) (and so inside the naturally aligned 16-byte granules that hold a byte of it), whatever the
 * alignment of base; with n == 0 base is not dereferenced.  Arrays are read and written for exactly the element counts
 * given below. */
/* The walk.  *nrec (a device word, required) = what kvsep_log_walk(buf, n, ...) returns for the same bytes.  off / len /
 * stored / type are each nullable and each written for exactly cap elements: element i < min(*nrec, cap) holds what the
 * host walk gives for record i, every element from there to cap is 0.  Records past cap are not stored; *nrec > cap
 * says the arrays were cut (as *nbad > bad_cap does in the list forms).  The padding has len == 0, so the arrays go to
 * kvsep_log_verify_device(count = cap) as they are: a block of length 0 is never dereferenced there. */
int kvsep_log_walk_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n, uint64_t* off,
                          uint64_t* len, uint32_t* stored, uint8_t* type, uint64_t cap, uint64_t* nrec);
/* The accept rule.  off, len, type and *nrec as the walk above wrote them for the same image (read at indices below
 * min(*nrec, cap) only); ok has cap bytes.  accept (required) and gap (nullable) are written for exactly cap elements,
 * 0 at and past min(*nrec, cap); *dropped and *bad_length_bytes are nullable device words.  The outputs equal those of
 * kvsep_log_accept_gaps(buf, n, ok, count = min(*nrec, cap), ...) byte for byte: *dropped its return value,
 * *bad_length_bytes its out-parameter. */
int kvsep_log_accept_gaps_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n,
                                 const uint64_t* off, const uint64_t* len, const uint8_t* type, const uint8_t* ok,
                                 const uint64_t* nrec, uint64_t cap, uint8_t* accept, uint8_t* gap, uint64_t* dropped,
                                 uint64_t* bad_length_bytes);
/* The whole reader: the walk, kvsep_log_verify_device(count = cap, total_bytes = n, max_len = 32762) and the accept
 * rule, chained on `stream` with no host step.  off, len, stored, type, ok and accept are required here (cap != 0);
 * ok[i] at and past the records is 0 (Value("") = 0 and Unmask(0) != 0). */
int kvsep_log_read_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n, uint64_t* off,
                          uint64_t* len, uint32_t* stored, uint8_t* type, uint8_t* ok, uint8_t* accept, uint8_t* gap,
                          uint64_t cap, uint64_t* nrec, uint64_t* dropped, uint64_t* bad_length_bytes);

/* ---------------------------------------------------------------- value-log reader on the device
 * kvsep_vlog_walk and the totals of kvsep_vlog_verify_host for a vlog image that is on the device (the output of
 * kvsep_vlog_frame_auto_device, say), so that walk -> checksum -> verdict runs on one stream with no host step and can
 * be captured.  vlog records lie back to back, so the position of each header is known only from the one before it: one
 * wavefront follows the chain through a window of the image staged in LDS, a global round trip per window instead of
 * per record.  An image of very many tiny records is therefore one wavefront for a long time (known bad
 * cases).  ABI 4 gained them as new entry points only.
 * Every array is a DEVICE pointer; every call is asynchronous on `stream`; no atomics.  Refused with KVSEP_EINVAL
 * before any device is touched: a null ctx, a null base with n != 0, a null nrec, cap > 2^32 - 1, and in the read form
 * a null off / len / stored / crc with cap != 0.
 * Memory touched: the image is never written; it is read in naturally aligned 16-byte granules that each hold at least
 * one byte of [base, base + n), whatever the alignment of base; with n == 0 base is not dereferenced. */
/* The walk.  *nrec (a device word, required) and *consumed (nullable) = what kvsep_vlog_walk(buf, n, ...) returns and
 * writes for the same bytes.  off / len / stored are each nullable and each written for exactly cap elements: element
 * i < min(*nrec, cap) holds what the host walk gives for record i; every element from there to cap is padding, off =
 * len = 0 and stored = kvsep_crc32c_mask(0), an empty block that passes kvsep_crc32c_verify_device(count = cap) and is
 * never dereferenced there.  cap == 0 with null arrays is the counting call; *nrec > cap says the arrays were cut.  Like
 * the host walk it does not stop at a bad checksum.  One kernel, no scratch: it can always be captured. */
int kvsep_vlog_walk_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n, uint64_t* off,
                           uint64_t* len, uint32_t* stored, uint64_t cap, uint64_t* nrec, uint64_t* consumed);
/* The whole reader: the walk, kvsep_crc32c_verify_device(count = cap, total_bytes = n, max_len = max_len_hint ?
 * max_len_hint : n) with expected_masked = stored and out = crc, the ok[] pass of kvsep_crc32c_verify_list_device when
 * ok (cap bytes, nullable) is given, and the totals, chained on `stream` with no host step.  off, len, stored and crc
 * are required when cap != 0.  *first_bad / *nbad (nullable) are the verify call's words: the padding passes, so they
 * speak of records only.  With c = min(*nrec, cap) and g = the leading records among the first c that pass, the
 * nullable device words receive *ngood = g, *good_bytes = g ? off[g-1] + len[g-1] : 0 and *drop_bytes = g < c ? len[g]
 * : 0 -- with *nrec <= cap exactly kvsep_vlog_verify_host's outputs.
 * Scratch: what the checksum step needs.  After kvsep_crc32c_reserve(ctx, count >= cap, total_bytes >= n) the call
 * allocates nothing and can be captured; a captured call larger than the reservation fails with KVSEP_EINVAL before
 * anything is enqueued. */
int kvsep_vlog_read_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n, uint64_t* off,
                           uint64_t* len, uint32_t* stored, uint32_t* crc, uint8_t* ok, uint64_t cap,
                           uint64_t max_len_hint, uint64_t* nrec, uint64_t* consumed, uint64_t* first_bad,
                           uint64_t* nbad, uint64_t* ngood, uint64_t* good_bytes, uint64_t* drop_bytes);

/* Record assembly on the device: which physical records join into the logical records log::Reader::ReadRecord returns
 * (the loop documented at kvsep_log_accept_gaps below).  Consecutive records form a CHAIN: a record that does not
 * continue the record in progress -- a rejected record, a FULL, a FIRST, a MIDDLE / LAST with gap set or with nothing in
 * progress, an unknown type -- starts a new one, so the chains cut [0, count) into runs.  A chain is WHOLE, a record the
 * reader returns, iff it is one accepted FULL or ends with a LAST that continued; its records are then the fragments, in
 * order.  Every other chain (a lone rejected record, a FIRST cut off by a gap, a MIDDLE with nothing before it, a record
 * still open at count) is dropped.  first[] / whole[] are the `first` and `keep` of kvsep_crc32c_offsets_device, and
 * first[] / frag_off[] / frag_len[] the first / seg_off / seg_len of kvsep_crc32c_pack_device and
 * kvsep_crc32c_gather_device, as they are.  ABI 4 gained these as new entry points only. */
/* Host, pure, no device: returns the number of chains.  type / accept / gap (nullable: all zero) have count elements;
 * first has count + 1: first[j] = the first record of chain j, and `count` in every element from nchain to count; whole
 * has count: whole[j] = 1 for a whole chain, 0 else and at and past nchain; *nwhole (nullable) = the whole chains. */
uint64_t kvsep_log_chains(const uint8_t* type, const uint8_t* accept, const uint8_t* gap, uint64_t count,
                          uint64_t* first, uint8_t* whole, uint64_t* nwhole);
/* The chains pass on the device, asynchronous on `stream`; all pointers are device pointers.  count = min(*nrec, cap);
 * type / accept / gap (nullable: all zero) / off / len are read at indices below count only.  first (cap + 1 elements),
 * whole (cap), *nchain (required) and *nwhole (nullable) equal kvsep_log_chains for that count element for element:
 * first holds `count` from nchain to cap, whole 0 from nchain to cap.  off / len / frag_off / frag_len are all four given
 * or all four null: frag_off[i] = off[i] + 1 and frag_len[i] = len[i] - 1 for i < count (the walk's off is the type byte,
 * its len 1 + payload; a len of 0, which no walk gives, yields 0), both 0 from count to cap.  Every array is written for
 * exactly the stated element count.  Three small kernels ordered by the stream (no atomics) on a few scratch words per
 * 1,024 records, sized by kvsep_crc32c_reserve(ctx, count >= cap, ...): a reserved call allocates nothing and can be
 * captured; a captured call larger than the reservation fails with KVSEP_EINVAL before anything is enqueued.  Refused
 * with KVSEP_EINVAL before any device is touched: a null ctx, a null type / accept / first / whole with cap != 0, some
 * but not all of off / len / frag_off / frag_len, a null nrec, a null nchain, cap > 2^32 - 1. */
int kvsep_log_chains_device(kvsep_crc32c_ctx* ctx, void* stream, const uint8_t* type, const uint8_t* accept,
                            const uint8_t* gap, const uint64_t* off, const uint64_t* len, const uint64_t* nrec,
                            uint64_t cap, uint64_t* first, uint8_t* whole, uint64_t* frag_off, uint64_t* frag_len,
                            uint64_t* nchain, uint64_t* nwhole);
/* The whole reader down to record bytes, chained on `stream` with no host step: kvsep_log_read_device (gap required
 * here), the chains pass, the offsets pass (seg_len = frag_len, first, keep = whole, head = tail = start = 0, count = nseg
 * = cap) and the plain gather-copy with the same descriptors.  dst receives the records log::Reader returns, back to
 * back from offset 0, in order; rec_off[j] (cap words) = where chain j's record went, KVSEP_OFFSET_SKIP for a chain that
 * is not whole or lies past *nchain; rec_len[j] (nullable, cap words) = the record's byte count when whole[j], else 0;
 * *end = the bytes needed, *nwhole (nullable) = the records.  The destination contract is kvsep_crc32c_salvage_device's:
 * a record that does not lie inside [0, dst_bytes) is not written, *end says what was needed, no byte of dst at or past
 * *end is written.  *nrec > cap says the arrays were cut: the result is then the assembly of the first cap physical
 * records, a chain open at the cut dropped as at the end of an image; read again with a larger cap.
 * kvsep_crc32c_reserve(ctx, count >= max(cap, ceil(n / 32768)), total_bytes >= n) makes the call allocation-free and
 * capturable; a captured call over the reservation is refused before its first kernel. */
int kvsep_log_records_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, uint64_t n, uint64_t* off,
                             uint64_t* len, uint32_t* stored, uint8_t* type, uint8_t* ok, uint8_t* accept, uint8_t* gap,
                             uint64_t cap, uint64_t* nrec, uint64_t* dropped, uint64_t* bad_length_bytes,
                             uint64_t* frag_off, uint64_t* frag_len, uint64_t* first, uint8_t* whole, uint64_t* nchain,
                             void* dst, uint64_t dst_bytes, uint64_t* rec_off, uint64_t* rec_len, uint64_t* end,
                             uint64_t* nwhole);

/* ---------------------------------------------------------------- batched host form
 * Host pointers. Blocks are gathered into pinned staging, copied H2D, checksummed and the
 * u32 results copied back, double-buffered over two streams; blocking. */
int kvsep_crc32c_batch_host(kvsep_crc32c_ctx* ctx, const uint32_t* init, const char* const* ptr,
                            const uint64_t* len, uint32_t* out, uint64_t count);
/* One contiguous host buffer (a vlog file image or a block buffer headed for pwrite):
 * out[i] = Extend(init?init[i]:0, host_base + off[i], len[i]). Blocking. */
int kvsep_crc32c_batch_host_span(kvsep_crc32c_ctx* ctx, const char* host_base, uint64_t span_bytes,
                                 const uint64_t* off, const uint64_t* len, const uint32_t* init, uint32_t* out,
                                 uint64_t count);

/* ---------------------------------------------------------------- framings (batched call sites)
 * vlog records (db/value_log_writer.cc:46-76, db/value_log_reader.cc:86-138):
 *   [Mask(Value(payload)) LE32][len LE32][payload], back to back from offset 0. */
/* Header walk: fills off/len/stored (nullable) for up to `cap` complete records; returns the number of
 * complete records; a truncated header or payload ends the walk (the reader's eof). */
uint64_t kvsep_vlog_walk(const char* buf, uint64_t n, uint64_t* off, uint64_t* len, uint32_t* stored, uint64_t cap,
                         uint64_t* consumed);
/* Recovery / GC scan: walk + one batched GPU checksum + compare.  *ngood = records before the first checksum
 * mismatch (the reader reports "checksum mismatch" there and stops), *good_bytes = end offset of the last good one,
 * *drop_bytes = the byte count VlogReader reports with that "checksum mismatch" (the bad record's payload length,
 * db/value_log_reader.cc:117-120), 0 when every complete record is intact.  Any output may be null. */
int kvsep_vlog_verify_host(kvsep_crc32c_ctx* ctx, const char* buf, uint64_t n, uint64_t* nrecords, uint64_t* ngood,
                           uint64_t* good_bytes, uint64_t* drop_bytes);
/* Group-commit write side: frames `count` payloads into dst (needs sum(8 + len) bytes, *written). */
int kvsep_vlog_frame_host(kvsep_crc32c_ctx* ctx, const char* const* payload, const uint64_t* len, uint64_t count,
                          char* dst, uint64_t dst_cap, uint64_t* written);
/* log / MANIFEST physical records (db/log_reader.cc:189-272): 32 KiB blocks of [crc LE32][len LE16][type][payload],
 * crc = Mask(Value(type || payload)).  Walk returns off = header + 6 (the type byte), len = 1 + payload length. */
uint64_t kvsep_log_walk(const char* buf, uint64_t n, uint64_t* off, uint64_t* len, uint32_t* stored, uint8_t* type,
                        uint64_t cap);
int kvsep_log_verify_host(kvsep_crc32c_ctx* ctx, const char* buf, uint64_t n, uint8_t* ok, uint64_t cap,
                          uint64_t* nrecords);
/* Device-resident form of the checksum step of kvsep_log_verify_host: base is the log image on the device, off / len /
 * stored the arrays kvsep_log_walk produced, copied to the device; ok[i] (device, u8, exactly `count` written) =
 * (Value(type || payload) == Unmask(stored[i])), the verdict kvsep_log_accept consumes.  Asynchronous on `stream`;
 * total_bytes / max_len are hints as in kvsep_crc32c_batch_device; scratch sized by kvsep_crc32c_reserve. */
int kvsep_log_verify_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                            const uint64_t* len, const uint32_t* stored, uint8_t* ok, uint64_t count,
                            uint64_t total_bytes, uint64_t max_len);
/* log / MANIFEST write side (db/log_writer.cc:35-115): appends `count` records to a log of current length
 * dest_length (the writer's block_offset_ = dest_length % 32 KiB, log_writer.cc:27-28), fragmenting each record
 * over 32 KiB blocks as FULL / FIRST / MIDDLE / LAST physical records and zero-filling block trailers of
 * fewer than 7 bytes; every fragment's crc = Mask(Extend(Value(&type, 1), fragment)) comes from ONE batched
 * call.  dst receives the appended bytes; *written = their count (also on KVSEP_EINVAL for a short dst). */
int kvsep_log_frame_host(kvsep_crc32c_ctx* ctx, const char* const* payload, const uint64_t* len, uint64_t count,
                         uint64_t dest_length, char* dst, uint64_t dst_cap, uint64_t* written);
/* Where that writer puts `count` records of len[i] bytes appended to a log of dest_length bytes.  Host, pure, no device.
 * keep (nullable: every record kept) drops record i when keep[i] == 0: it is not written and changes nothing.
 *   rec_at[i]     (count)     = the offset of record i's first header, relative to the first appended byte;
 *                               KVSEP_OFFSET_SKIP for a dropped record,
 *   frag_first[i] (count + 1) = the physical records (fragments) of the records before i; frag_first[count] = *nfrag,
 *   *written                  = the appended bytes (what kvsep_log_frame_host reports for the kept records).
 * The zero trailer of a block with fewer than 7 bytes left belongs to the NEXT kept record, as in the writer: none
 * follows the last record, and dest_length % 32768 > 32761 puts one in front of the first.  A kept empty record is one
 * 7-byte FULL header.  *nfrag <= 2 * kept + total_bytes / 32761 (a record has one fragment, one more for the block it
 * starts in when it does not fit, and one per further 32,761 bytes), which sizes frag_cap and, with *written, dst.
 * Sums saturate at 2^64 - 1 as in kvsep_crc32c_offsets_device: a kept record whose end saturates, and every kept record
 * after it, gets KVSEP_OFFSET_SKIP and owns no fragment, and *written = 2^64 - 1.  Returns KVSEP_EINVAL for a null
 * frag_first, or a null len / rec_at with count != 0; nfrag and written are nullable.  ABI 4 gained this and
 * kvsep_log_frame_device as new entry points only. */
int kvsep_log_frame_layout(const uint64_t* len, const uint8_t* keep, uint64_t count, uint64_t dest_length,
                           uint64_t* rec_at, uint64_t* frag_first, uint64_t* nfrag, uint64_t* written);
/* The write side on the device, asynchronous on `stream`; every array is a device pointer.  Record i is the bytes
 * [base + off[i], + len[i]); a dropped record (keep[i] == 0; keep nullable) is never dereferenced whatever its off, so
 * rec_off / rec_len / whole of kvsep_log_records_device go in as off / len / keep with count = cap.  Lengths are trusted
 * as in kvsep_crc32c_batch_device.  dst[0, dst_bytes) receives the appended bytes from offset 0: headers, fragments and
 * zero trailers, byte for byte what kvsep_log_frame_host writes for the kept records.  rec_at (count), frag_first
 * (count + 1), *nfrag and *written (all three required) equal kvsep_log_frame_layout.  Per fragment slot f < frag_cap,
 * each array written for exactly frag_cap elements:
 *   frag_off[f] / frag_len[f] = the fragment's bytes (an offset from base; at most 32,761 bytes),
 *   frag_at[f]   = its header's offset in dst,   frag_type[f] = 1 FULL, 2 FIRST, 3 MIDDLE, 4 LAST,
 *   frag_crc[f]  = Extend(Value(&type, 1), fragment), unmasked (the header stores Mask of it),
 * and 0 / 0 / KVSEP_OFFSET_SKIP / 0 / 0 at and past min(*nfrag, frag_cap).  *nfrag > frag_cap says the fragment arrays
 * were cut: fragments at or past frag_cap are not written to dst, nor is the zero trailer in front of a record whose
 * first fragment is; call again with a larger cap.  A fragment (header and bytes) that does not lie inside
 * [0, dst_bytes) is not written at all, and neither is a trailer; *written says what was needed, and no byte of dst at
 * or past *written is written.  total_bytes is the hint of the checksum pass (the kept bytes).
 * Two small kernels (the layout: one wavefront, 64 records a step; the fragment fill), the batched checksum with
 * max_len 32,761 and the gather-copy with the log frame, ordered by the stream, no atomics; scratch is one word per
 * record and per fragment slot.  kvsep_crc32c_reserve(ctx, count >= max(count, frag_cap), total_bytes) makes the call
 * allocation-free and capturable; a captured call over the reservation is refused before its first kernel.  Refused with
 * KVSEP_EINVAL before any device is touched: a null ctx; a null base / off / len / rec_at with count != 0; a null
 * fragment array or dst with frag_cap != 0; a null frag_first, nfrag or written; count or frag_cap over 2^32 - 1. */
int kvsep_log_frame_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                           const uint64_t* len, const uint8_t* keep, uint64_t count, uint64_t dest_length, void* dst,
                           uint64_t dst_bytes, uint64_t* rec_at, uint64_t* frag_first, uint64_t* frag_off,
                           uint64_t* frag_len, uint64_t* frag_at, uint8_t* frag_type, uint32_t* frag_crc,
                           uint64_t frag_cap, uint64_t* nfrag, uint64_t* written, uint64_t total_bytes);
/* What log::Reader::ReadPhysicalRecord returns, given the walk (off as from kvsep_log_walk) and each record's
 * checksum verdict ok[i]: a mismatch drops the rest of its 32 KiB block buffer (db/log_reader.cc:250-258), so
 * that record and every later record of the same block get accept[i] = 0.  Returns the bytes reported as
 * dropped with "checksum mismatch" (header of the bad record to the end of its block, or of the file). */
uint64_t kvsep_log_accept(const uint64_t* off, const uint8_t* ok, uint64_t count, uint64_t n, uint8_t* accept);
/* kvsep_log_accept plus the reader events that leave no physical record behind.  ReadPhysicalRecord also returns
 * kBadRecord, without a checksum, for a record length past its block ("bad record length", db/log_reader.cc:224-230)
 * and for a preallocated zero header (:237-243); kvsep_log_walk only stops walking that block there.  In ReadRecord
 * every kBadRecord abandons a fragmented record in progress (:153-159), so a caller that assembles FIRST / MIDDLE /
 * LAST fragments from accept[] alone can join fragments across such a hole into a record log::Reader never returns.
 * This call re-reads the headers of the host image buf[0, n) (the image kvsep_log_walk walked; ok[i] / count = its
 * records and their checksum verdicts) and gives, besides accept[i] and the return value of kvsep_log_accept,
 *   gap[i] (nullable) = 1 when such an event lies between record i-1 and record i: reset the assembly before record i;
 *   *bad_length_bytes (nullable) = the bytes the reader reports with "bad record length" (only for blocks read in
 *   full: in a short last block the reader takes a long record for a torn write, :231-234).
 * It also knows the two type bytes that ReadPhysicalRecord's return value (:270-271, the type byte itself) turns into
 * the reader's own codes (db/log_reader.h:66,72): a record of type 5 with a good checksum reads as kEof, so log::Reader
 * stops there -- accept = 0 for it and for every later record, and nothing after it is counted; type 6 reads as a
 * kBadRecord nobody reports -- accept = 0.  kvsep_log_accept, which sees no types, accepts both.
 * Assembly, as log::Reader::ReadRecord does it (type[] from kvsep_log_walk; payload i = [off[i] + 1, off[i] + len[i])):
 *   for each i:  if (gap[i] || !accept[i]) drop the record in progress;
 *                if (!accept[i]) continue;
 *                FULL: drop the record in progress, return payload i;   FIRST: start a record with payload i;
 *                MIDDLE / LAST: if a record is in progress, append payload i (LAST: and return it);
 *                any other type: drop the record in progress ("unknown record type").
 *   A record still in progress at the end of the image is dropped (:144-151). */
uint64_t kvsep_log_accept_gaps(const char* buf, uint64_t n, const uint8_t* ok, uint64_t count, uint8_t* accept,
                               uint8_t* gap, uint64_t* bad_length_bytes);
/* SST block trailers (table/table_builder.cc:209-232): masked_out[i] = Mask(Extend(Value(block_i), &types[i], 1)),
 * the LE32 word written after the type byte.  Device pointers, async on stream. */
int kvsep_sst_trailers_device(kvsep_crc32c_ctx* ctx, void* stream, const void* base, const uint64_t* off,
                              const uint64_t* len, const uint8_t* types, uint32_t* masked_out, uint64_t count,
                              uint64_t total_bytes, uint64_t max_len);
/* SST block read check (table/format.cc:99-106): the file image holds [block][type][trailer word]; out[i] =
 * Value(block, len + 1) (= Unmask(stored) when intact); *first_bad / *nbad as in kvsep_crc32c_verify_device. */
int kvsep_sst_verify_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, const uint64_t* off,
                            const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count,
                            uint64_t total_bytes, uint64_t max_len);
/* List form of the read check: as kvsep_sst_verify_device, plus bad_idx / bad_cap / ok as in
 * kvsep_crc32c_verify_list_device -- every block ReadBlock would report as "block checksum mismatch", by index: the
 * call for RepairDB::ScanTable (db/repair.cc:220-260) and paranoid compaction inputs, which skip those and keep the
 * rest. */
int kvsep_sst_verify_list_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, const uint64_t* off,
                                 const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad,
                                 uint64_t* bad_idx, uint64_t bad_cap, uint8_t* ok, uint64_t count, uint64_t total_bytes,
                                 uint64_t max_len);
/* Host-resident forms of the two above, for blocks the way TableBuilder::WriteRawBlock (table/table_builder.cc:209-232)
 * and ReadBlock (table/format.cc:73-108) hold them: in host memory.  Both go through the pinned staging pipeline of
 * the host forms; blocking.
 *   trailers: block[i] / len[i] host pointers, types[i] the compression type byte; masked_out[i] =
 *             Mask(Extend(Value(block_i), &types[i], 1)).
 *   verify:   `file` is an SST file image in host memory ([block][type][trailer word] at each handle off[i] / len[i];
 *             KVSEP_EINVAL if a handle leaves no room for its 5-byte trailer, format.cc:84-87); out[i] =
 *             Value(block, len + 1); *first_bad = lowest i whose out[i] != Unmask(stored word) (UINT64_MAX if none),
 *             *nbad their number -- each such block is what ReadBlock reports as "block checksum mismatch". */
int kvsep_sst_trailers_host(kvsep_crc32c_ctx* ctx, const char* const* block, const uint64_t* len, const uint8_t* types,
                            uint32_t* masked_out, uint64_t count);
int kvsep_sst_verify_host(kvsep_crc32c_ctx* ctx, const char* file, uint64_t n, const uint64_t* off, const uint64_t* len,
                          uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count);
/* kvsep_sst_verify_host plus the list (host array bad_idx, at most bad_cap entries, ascending; NULL iff bad_cap == 0):
 * the same handle checks; the image is copied to the device for the call and the list comes from the device pass of
 * kvsep_sst_verify_list_device, not from a second compare on the host.  Blocking; KVSEP_ENOMEM if the image does not
 * fit in device memory. */
int kvsep_sst_verify_list_host(kvsep_crc32c_ctx* ctx, const char* file, uint64_t n, const uint64_t* off,
                               const uint64_t* len, uint32_t* out, uint64_t* first_bad, uint64_t* nbad,
                               uint64_t* bad_idx, uint64_t bad_cap, uint64_t count);

/* ---------------------------------------------------------------- SST table reader: footer, index walk, whole table
 * Where the block handles of the forms above come from: the footer (Footer::DecodeFrom, table/format.cc:37-60) and the
 * walk of the index block (Block::Block, DecodeEntry, Block::Iter, table/block.cc; BlockHandle::DecodeFrom), on the
 * host and for a table image that is on the device, so that a device-resident table goes from bytes to a per-block
 * verdict list on one stream with no host step.  ABI 4 gained them as new entry points and defines only.
 *
 * The status word of every form holds one of: */
#define KVSEP_SST_OK 0
#define KVSEP_SST_BAD_FOOTER 1       /* n < 48, wrong magic, a varint that leaves the 40 bytes, an unusable handle */
#define KVSEP_SST_INDEX_CHECKSUM 2   /* table form: the index block failed its read check; no handle of it is trusted */
#define KVSEP_SST_INDEX_COMPRESSED 3 /* table form: the index block's type byte is not 0 (Snappy is not rebuilt here) */
#define KVSEP_SST_BAD_RESTARTS 4     /* block shorter than 4, restart count too large for it (or for the reserved
                                        scratch), restart[0] != 0, a restart not above the one before or not below
                                        the restart array */
#define KVSEP_SST_BAD_ENTRY 5        /* an entry header that does not decode or leaves its restart run, shared != 0 on
                                        a run's first entry, shared above the previous key's length */
#define KVSEP_SST_BAD_HANDLE 6       /* an entry's value does not hold two varint64 */
#define KVSEP_SST_CAP 7              /* table form: *nblocks + 2 > cap, the slots do not hold every block */
/* A handle (off, len) is usable in an image of n bytes iff off + len + 5 <= n (no sum wraps): the block and its 5-byte
 * trailer lie inside.
 * First error wins: the result is the entries of all restart runs before the lowest run with an error, plus that run's
 * entries before its error, in order; status is that error's code and *nblocks counts exactly those entries.  A run
 * whose next restart is bad is walked to the end of the entries.  On a block with no error the result is what
 * Block::Iter yields from SeekToFirst to the end.  A decoded handle that is not usable is still emitted; whether it may
 * be dereferenced is decided where it is used. */
/* The footer of an image of n bytes: handles = {meta_off, meta_len, index_off, index_len}, all 0 unless *status is
 * KVSEP_SST_OK.  Host memory; returns KVSEP_EINVAL for a null pointer (file may be null when n == 0). */
int kvsep_sst_footer(const char* file, uint64_t n, uint64_t handles[4], uint32_t* status);
/* The walk of one index block's contents blk[0, blk_len) (without its trailer).  off / len (nullable when cap == 0) are
 * written for exactly cap elements, zero from min(*nblocks, cap) on; *nblocks is the full count even when cap cut the
 * arrays (status stays what the walk found).  Host memory. */
int kvsep_sst_index_walk(const char* blk, uint64_t blk_len, uint64_t* off, uint64_t* len, uint64_t cap,
                         uint64_t* nblocks, uint32_t* status);
/* The device forms.  Every pointer except ctx is DEVICE memory; nothing is read back; asynchronous on `stream`; results
 * are identical from run to run (no atomics).  The argument refusals come before the context or any device is touched:
 * a null file_base with n != 0, a null required pointer, cap > 2^32 - 1, cap < 2 in the table form -- each KVSEP_EINVAL.
 * A lane walks a restart run, so the reference's index blocks (block_restart_interval = 1) walk fully in parallel; one
 * run of very many entries is one lane's chain of dependent loads.
 * Scratch: two words per restart run (and one per 256 of them) plus the offsets pass's, and the SST arrays for cap.
 * The restart count is device data, so the walk handles as many runs as its scratch holds: the largest count given to
 * kvsep_crc32c_reserve, or cap when that is more (an eager call allocates for it; a captured call over the reservation
 * fails with KVSEP_EINVAL before anything is enqueued).  A block with more runs than that stops with
 * KVSEP_SST_BAD_RESTARTS and *nblocks = 0; nothing is written past the scratch.
 * kvsep_crc32c_reserve(ctx, count >= max(cap, index_len / 4), total_bytes >= n) makes a call allocation-free and
 * capturable, and is the sizing to use: index_len / 4 bounds the restart count of that block, and cap alone is enough
 * for a table whose blocks all fit the slots at restart interval 1.  Without any knowledge of the table count = n / 4
 * is always enough, but reserve sizes every per-block array of the library for count (on the order of 100 bytes a
 * block: several GiB for a 258 MiB image).  A call launches lanes for the runs its scratch holds, never for more than
 * n / 4.
 * Memory touched: the image is never written; it is read bytewise, in the last 48 bytes, inside
 * [index_off, index_off + index_len + 5) and, in the table form, at the blocks and trailers of usable handles -- so
 * every read lies inside [file_base, file_base + n). */
/* The walk alone.  handle[0..2) = index_off, index_len (an unusable one gives KVSEP_SST_BAD_FOOTER); off / len / cap /
 * *nblocks / *status as kvsep_sst_index_walk gives them for the block's bytes. */
int kvsep_sst_index_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, uint64_t n,
                           const uint64_t* handle, uint64_t* off, uint64_t* len, uint64_t cap, uint64_t* nblocks,
                           uint32_t* status);
/* The whole table: the footer (handles[4], as kvsep_sst_footer), the read check of the index block alone, its walk,
 * then the read check and list pass of kvsep_sst_verify_list_device over all cap >= 2 slots: crc / first_bad / nbad /
 * bad_idx / bad_cap / ok as there, with count = cap.  Slots [0, m) are the data blocks in index order, m =
 * min(*nblocks, cap - 2); slot m is the metaindex block, slot m + 1 the index block; the rest is padding (off = len = 0,
 * checked as a block of length 0 that passes: ok = 1, not counted in *nbad).  *nblocks + 2 > cap sets KVSEP_SST_CAP.
 * An index block that fails its checksum gives KVSEP_SST_INDEX_CHECKSUM, one whose type byte is not 0
 * KVSEP_SST_INDEX_COMPRESSED (its checksum still reported): *nblocks = 0 and the list holds the metaindex and index
 * blocks only.  A bad footer lists nothing.  Data blocks may be compressed: the check covers the stored bytes and the
 * type byte.  An emitted handle that is not usable is reported bad (crc = 0) and never dereferenced.  max_len_hint: the
 * longest block (0 = unknown), a hint only.  off / len / crc / ok go to kvsep_sst_salvage_device as they are. */
int kvsep_sst_table_verify_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, uint64_t n, uint64_t* off,
                                  uint64_t* len, uint32_t* crc, uint64_t* first_bad, uint64_t* nbad, uint64_t* bad_idx,
                                  uint64_t bad_cap, uint8_t* ok, uint64_t cap, uint64_t max_len_hint,
                                  uint64_t* nblocks, uint64_t* handles, uint32_t* status);

/* ---------------------------------------------------------------- SST table writer: index block build, table rewrite
 * The write side of the reader above: kvsep_sst_salvage_device leaves the blocks that passed back to back with their
 * trailers, which is not a table -- it has no index block, no metaindex block and no footer.  These forms finish it on
 * the same stream with no host step.  ABI 4 gained them as new entry points and defines only.
 *
 * Two facts make the rewrite correct without looking inside data blocks: an index entry's key is a separator (>= every
 * key of its block, < the first key of the next), and dropping entry j leaves every remaining separator valid for the
 * blocks that remain.  So the new index is the kept entries' key bytes, copied from the old index block, with the new
 * handles.  The reference writes index blocks at block_restart_interval = 1 (table/table_builder.cc:36,92): every key
 * is stored whole and contiguous.  Expanding prefix-compressed keys is not built: */
#define KVSEP_SST_SHARED_KEY 8       /* keys walk: an entry shares key bytes with the one before it (shared != 0), so
                                        its key has no contiguous place in the block */
/* The walk, with keys: kvsep_sst_index_walk / kvsep_sst_index_device with two more outputs, under the same rules (first
 * error wins; outputs written for exactly cap elements, zero from min(*nblocks, cap) on; *nblocks the full count).
 * key_off[i] is the offset of entry i's key bytes (host form: in blk; device form: in the image) and key_len[i] their
 * length.  An entry with shared != 0 stops the walk with KVSEP_SST_SHARED_KEY; the entries before it are emitted. */
int kvsep_sst_index_keys(const char* blk, uint64_t blk_len, uint64_t* off, uint64_t* len, uint64_t* key_off,
                         uint64_t* key_len, uint64_t cap, uint64_t* nblocks, uint32_t* status);
int kvsep_sst_index_keys_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, uint64_t n,
                                const uint64_t* handle, uint64_t* off, uint64_t* len, uint64_t* key_off,
                                uint64_t* key_len, uint64_t cap, uint64_t* nblocks, uint32_t* status);
/* The status word of the builder forms: */
#define KVSEP_SSTW_OK 0
#define KVSEP_SSTW_TOO_LARGE 1 /* the block would reach 2^32 bytes (restart offsets are 32-bit), or a key_len exceeds
                                  2^32 - 1; sums saturate as in the offsets pass */
#define KVSEP_SSTW_NO_ROOM 2   /* position + block + 5 (the table form: + 13 before and + 48 after) > dst_bytes */
#define KVSEP_SSTW_SOURCE 3    /* rewrite only: the source's status is KVSEP_SST_BAD_FOOTER, _INDEX_CHECKSUM,
                                  _INDEX_COMPRESSED or _SHARED_KEY: there is no index to rewrite */
/* The index block BlockBuilder produces at restart interval 1 for the kept entries in order, with its trailer:
 *   entry i is kept iff keep[i] != 0 (or keep is null) and blk_off[i] != KVSEP_OFFSET_SKIP -- the salvage's ok[] and
 *   dst_off[] go in as they are; its key is key_base[key_off[i], + key_len[i]), its value the handle (blk_off[i],
 *   blk_len[i]);
 *   entries: varint32(0) varint32(key_len) varint32(value_len) key varint64(off) varint64(len); then restart[k] = byte
 *   position of the k-th kept entry (LE32) and the restart count; with no kept entry the reference's empty block, one
 *   restart of 0 and a count of 1 (8 bytes);
 *   the trailer [0][Mask(Extend(Value(block), "\0", 1)) LE32] follows; *out_len is the block's length without it.
 * The block goes to dst + at.  On a refusal nothing is written and *out_len holds the needed length (0 when too large).
 * Host form: host arrays, `at` a value.  Returns KVSEP_EINVAL for a null required pointer. */
int kvsep_sst_index_build(const char* key_base, const uint64_t* key_off, const uint64_t* key_len,
                          const uint64_t* blk_off, const uint64_t* blk_len, const uint8_t* keep, uint64_t count,
                          char* dst, uint64_t dst_bytes, uint64_t at, uint64_t* out_len, uint32_t* status);
/* The 48-byte footer (Footer::EncodeTo, table/format.cc:23-35): the metaindex and index handles as varint64s, zero
 * padding to 40 bytes, the magic. */
int kvsep_sst_footer_build(uint64_t meta_off, uint64_t meta_len, uint64_t index_off, uint64_t index_len, char out[48]);
/* The device forms.  Every pointer except ctx is DEVICE memory, `at` / `data_end` included (the position depends on a
 * salvage's *end; the kernels read it); nothing is read back; asynchronous on `stream`; no atomics, results identical
 * from run to run.  The argument refusals come before the context or any device is touched: a null required pointer,
 * count > 2^32 - 1 -- each KVSEP_EINVAL.  The refusals above are decided on the device from the totals before anything
 * is written.
 * Kernels: a size kernel, the offsets pass twice (byte positions; ranks among the kept), the fill kernel (a wavefront
 * stages its 64 entries in LDS and stores the range in aligned 16-B granules, byte stores at the edges; a range over
 * 4 KiB is written entry by entry by the whole wave), the batched checksum over the one block, a tail kernel.
 * Scratch: four words per entry plus the offsets pass's and a one-block plan: kvsep_crc32c_reserve(ctx, count,
 * total_bytes >= min(dst_bytes, 2^32)) makes a call allocation-free and capturable; a captured call over its
 * reservation fails with KVSEP_EINVAL before anything is enqueued.
 * Memory touched: key_off / key_len / blk_off / blk_len / keep are read for count elements; key bytes are read only
 * for kept entries, inside [key_off[i], key_off[i] + key_len[i]) -- when a wave's range is over 4 KiB, inside the
 * naturally aligned 16-B granules of key_base that hold such a byte; dst is written only inside the block and its
 * trailer, nothing is read-modify-written. */
int kvsep_sst_index_build_device(kvsep_crc32c_ctx* ctx, void* stream, const void* key_base, const uint64_t* key_off,
                                 const uint64_t* key_len, const uint64_t* blk_off, const uint64_t* blk_len,
                                 const uint8_t* keep, uint64_t count, void* dst, uint64_t dst_bytes, const uint64_t* at,
                                 uint64_t* out_len, uint32_t* status);
/* Finishes a table whose data blocks end at *data_end: the empty metaindex block with its trailer (13 bytes) at
 * *data_end, the index block above at *data_end + 13, the 48-byte footer after its trailer; *index_len as *out_len
 * above, *table_bytes the table's size (0 after a refusal, which writes nothing).  dst is written only inside
 * [*data_end, *table_bytes).  The output has no filter block: filter offsets are tied to the old layout, and
 * Table::Open accepts a table without one. */
int kvsep_sst_table_finish_device(kvsep_crc32c_ctx* ctx, void* stream, const void* key_base, const uint64_t* key_off,
                                  const uint64_t* key_len, const uint64_t* blk_off, const uint64_t* blk_len,
                                  const uint8_t* keep, uint64_t count, void* dst, uint64_t dst_bytes,
                                  const uint64_t* data_end, uint64_t* index_len, uint64_t* table_bytes,
                                  uint32_t* status);
/* Source image in, finished table out, on one stream: kvsep_sst_table_verify_device with the keys walk (off / len /
 * crc / ok / cap / max_len_hint / nblocks / handles / status as there; key_off / key_len have cap elements); a keep
 * mask of ok[i] for the data slots i < min(*nblocks, cap - 2); the salvage's layout (dst_off[cap], *nkept, nullable)
 * and copy; kvsep_sst_table_finish_device with blk_off = dst_off (index_len / table_bytes / wstatus as there).
 * A source status of KVSEP_SST_BAD_FOOTER, _INDEX_CHECKSUM, _INDEX_COMPRESSED or _SHARED_KEY writes nothing:
 * *table_bytes = 0, *wstatus = KVSEP_SSTW_SOURCE.  Any other entry error keeps the entries before it, as the salvage
 * does.  KVSEP_SST_CAP (more data blocks than cap - 2 slots) does not refuse either: the output is a finished table of
 * the first cap - 2 data blocks that passed, *wstatus is KVSEP_SSTW_OK, and *status / *nblocks are what tell the caller
 * that blocks past the slots were left out -- size cap from the index length to rule it out.  With every block good and the source laid out as TableBuilder lays it out without a filter policy (data blocks
 * back to back from 0, then the metaindex block), the output equals the source byte for byte.
 * Reserve as for the table verify and the builder: kvsep_crc32c_reserve(ctx, count >= max(cap, index_len / 4),
 * total_bytes >= max(n + cap, dst_bytes)). */
int kvsep_sst_table_rewrite_device(kvsep_crc32c_ctx* ctx, void* stream, const void* file_base, uint64_t n, void* dst,
                                   uint64_t dst_bytes, uint64_t* off, uint64_t* len, uint64_t* key_off,
                                   uint64_t* key_len, uint32_t* crc, uint8_t* ok, uint64_t* dst_off, uint64_t cap,
                                   uint64_t max_len_hint, uint64_t* nblocks, uint64_t* nkept, uint64_t* handles,
                                   uint32_t* status, uint64_t* index_len, uint64_t* table_bytes, uint32_t* wstatus);

/* ---------------------------------------------------------------- several GPUs in one process
 * Blocks are independent, so a batch is cut into contiguous block ranges balanced by bytes and each range runs on
 * its own device; payload never crosses between GPUs, only the u32 results come back (into ONE array).  For a
 * single KVDB process scanning whole vlogs (GC db/db_impl.cc:880-951, recovery :485-571) on every GPU it has. */
/* bounds[0..parts]: part p = blocks [bounds[p], bounds[p+1]), each ~sum(len)/parts bytes (the cut nearest to each
 * p/parts point of the prefix sum of len).  Host arrays; no device needed. */
int kvsep_crc32c_partition(const uint64_t* len, uint64_t count, int parts, uint64_t* bounds);
typedef struct kvsep_crc32c_group kvsep_crc32c_group;
/* One context (and stream) per listed device; a device may be listed twice (two independent contexts on it). */
int kvsep_crc32c_group_create(const int* devices, int ndev, kvsep_crc32c_group** out);
void kvsep_crc32c_group_destroy(kvsep_crc32c_group* g);
int kvsep_crc32c_group_size(kvsep_crc32c_group* g);
kvsep_crc32c_ctx* kvsep_crc32c_group_ctx(kvsep_crc32c_group* g, int i); /* member i's context (tuning knobs) */
/* kvsep_crc32c_batch_host_span over the whole group: part i through member i's pinned staging on its own PCIe link,
 * one host thread per member; blocking. */
int kvsep_crc32c_group_batch_host_span(kvsep_crc32c_group* g, const char* host_base, uint64_t span_bytes,
                                       const uint64_t* off, const uint64_t* len, const uint32_t* init, uint32_t* out,
                                       uint64_t count);
/* ... plus Mask(out[i]) == expected_masked[i]: *first_bad = lowest mismatching index (UINT64_MAX if none), *nbad. */
int kvsep_crc32c_group_verify_host_span(kvsep_crc32c_group* g, const char* host_base, uint64_t span_bytes,
                                        const uint64_t* off, const uint64_t* len, const uint32_t* init,
                                        const uint32_t* expected_masked, uint32_t* out, uint64_t* first_bad,
                                        uint64_t* nbad, uint64_t count);
/* ONE buffer over the whole group: *out = Extend(init_crc, data, n).  Member p of N checksums bytes
 * [floor(n p / N), floor(n (p + 1) / N)) -- cut wherever that falls, at any alignment -- as one block through its own
 * host-span pipeline (its pinned staging, its PCIe link, its host thread bound to its node), and the host joins the N
 * values with kvsep_crc32c_combine.  n == 0 gives init_crc; with n < N some parts are empty.  Blocking.  The one call a
 * single large Extend needs to use every GPU the process holds. */
int kvsep_crc32c_group_extend_host(kvsep_crc32c_group* g, uint32_t init_crc, const char* data, uint64_t n,
                                   uint32_t* out);
/* kvsep_vlog_verify_host with the checksums spread over the group. */
int kvsep_vlog_verify_host_group(kvsep_crc32c_group* g, const char* buf, uint64_t n, uint64_t* nrecords,
                                 uint64_t* ngood, uint64_t* good_bytes, uint64_t* drop_bytes);
/* Device-resident shards: member i's blocks live on ITS device (base[i], off[i], len[i], init[i] (nullable array or
 * entries), out[i] are device pointers there, count[i] blocks, total_bytes[i] / max_len[i] hints as in
 * kvsep_crc32c_batch_device).  Runs every shard on its member's stream and returns when all are done. */
int kvsep_crc32c_group_batch_device(kvsep_crc32c_group* g, const void* const* base, const uint64_t* const* off,
                                    const uint64_t* const* len, const uint32_t* const* init, uint32_t* const* out,
                                    const uint64_t* count, const uint64_t* total_bytes, const uint64_t* max_len);
/* ... verify form: shard i's block k is global block index_base[i] + k; *first_bad = the lowest global mismatching
 * index over all shards (UINT64_MAX if none), *nbad = the total -- the reduction SURVEY §8e puts on RCCL between
 * ranks, done here between the members of one process.  expected_masked may be NULL (then = batch_device). */
int kvsep_crc32c_group_verify_device(kvsep_crc32c_group* g, const void* const* base, const uint64_t* const* off,
                                     const uint64_t* const* len, const uint32_t* const* init,
                                     const uint32_t* const* expected_masked, uint32_t* const* out,
                                     const uint64_t* index_base, const uint64_t* count, const uint64_t* total_bytes,
                                     const uint64_t* max_len, uint64_t* first_bad, uint64_t* nbad);

/* ... list form: each member lists its shard's bad blocks on its device (kvsep_crc32c_verify_list_device); the host
 * merges the shard lists into global indices index_base[i] + k, ascending, into bad_idx[0 .. min(*nbad, bad_cap))
 * (a HOST array here, like first_bad / nbad; NULL iff bad_cap == 0).  *nbad is the total over all shards. */
int kvsep_crc32c_group_verify_list_device(kvsep_crc32c_group* g, const void* const* base, const uint64_t* const* off,
                                          const uint64_t* const* len, const uint32_t* const* init,
                                          const uint32_t* const* expected_masked, uint32_t* const* out,
                                          const uint64_t* index_base, const uint64_t* count,
                                          const uint64_t* total_bytes, const uint64_t* max_len, uint64_t* first_bad,
                                          uint64_t* nbad, uint64_t* bad_idx, uint64_t bad_cap);

/* ---------------------------------------------------------------- topology and host placement (round 5)
 * Which physical GPU a caller runs on, and the NUMA node its host legs belong on.  sysfs is read under
 * $KVSEP_SYSFS_ROOT (default /sys). */
/* PCI bus ID of a device ("0000:75:00.0", lower case, as sysfs spells it) into buf (len >= 13). */
int kvsep_device_pci_bus_id(int device, char* buf, int len);
/* NUMA node of a PCI function / of a device (sysfs numa_node), -1 when unknown. */
int kvsep_pci_numa_node(const char* pci_bus_id);
int kvsep_device_numa_node(int device);
/* CPUs of a NUMA node (sysfs cpulist) into cpus[0..cap); returns how many it has (0: unknown node). */
int kvsep_numa_node_cpus(int node, int* cpus, int cap);
/* Binds every thread of the calling process to the CPUs of `node` that the calling thread may run on, and makes
 * `node` the calling thread's preferred memory node (its later allocations, pinned host buffers included, land there
 * first).  Returns the number of CPUs bound to; 0 (nothing changed) for an unknown node or one that shares no CPU
 * with the current affinity.  For a process that drives one GPU (a bench rank): call it right after selecting the
 * device, before allocating pinned memory. */
int kvsep_bind_process_numa(int node);
/* NUMA node of the page holding p (faulted in if never touched), -1 if unknown. */
int kvsep_host_page_node(const void* p);

/* Pinned (page-locked) host memory for file images: read a vlog / SST file straight into it and the
 * host-span entry points DMA from it directly, without the staging memcpy.  NULL on failure. */
void* kvsep_host_alloc_pinned(uint64_t bytes);
void kvsep_host_free_pinned(void* p);

/* ---------------------------------------------------------------- support
 * Synthetic data: byte i of the stream is byte (i&7) of splitmix64 word (i>>3) of `seed`
 * (word j = mix(seed + (j+1)*0x9E3779B97F4A7C15)); writes bytes [stream_offset, +nbytes) to dst. */
int kvsep_fill_splitmix64_device(void* stream, void* dst, uint64_t nbytes, uint64_t seed, uint64_t stream_offset);
/* Read-only streaming kernel over [src, src+nbytes) (16-B loads, XOR-reduced into *sink):
 * the attainable HBM-read ceiling the CRC kernel is compared with. */
int kvsep_stream_read_device(kvsep_crc32c_ctx* ctx, void* stream, const void* src, uint64_t nbytes, uint32_t* sink);
const char* kvsep_last_error(void);
const char* kvsep_build_info(void);
int kvsep_device_count(void);

#ifdef __cplusplus
}  /* extern "C" */
#endif
#endif /* KVSEP_CRC32C_H_ */
