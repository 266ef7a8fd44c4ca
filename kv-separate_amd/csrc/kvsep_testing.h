// kvsep_testing.h -- test-only entry points of libkvsep_crc32c (not part of the public ABI, include/kvsep_crc32c.h).
// Exported so the test suite can reach them through ctypes, but inert unless the process runs with KVSEP_TEST_HOOKS=1
// (ADVICE r5): no production caller can make a batch call fail through them by accident.
#pragma once

#include "../../include/kvsep_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fault injection: the context's next batched call returns KVSEP_EHIP right after it enqueued its CRC kernel, before
 * the combine kernel of a planned batch -- the one point where an eager verify call's accumulators hold posts that no
 * kernel will publish.  The next verify call on the context resets them first, so its verdict is exact.  KVSEP_EINVAL
 * without KVSEP_TEST_HOOKS=1. */
int kvsep_crc32c_ctx_inject_failure(kvsep_crc32c_ctx* ctx);

/* What a batch call with these count / total_bytes / max_len hints would run as (read-only, needs no hook variable):
 * *piece_bytes the piece size (the automatic smaller sizes of small batches included), *pieces_needed the plan entries
 * the call asks its scratch for (0: no plan, every block unsplit) and *guided 1 for the guided schedule, 0 for the
 * static one.  Any of the three may be null.  The SST read check runs (count, total_bytes + count, max_len + 1).  Tests
 * assert with it that they hit the piece size and schedule they meant to. */
int kvsep_crc32c_plan_query(kvsep_crc32c_ctx* ctx, uint64_t count, uint64_t total_bytes, uint64_t max_len,
                            uint64_t* piece_bytes, uint64_t* pieces_needed, int* guided);

#ifdef __cplusplus
}
#endif
