// route.h -- which CRC kernel a batch runs on, and how (no HIP: tests/cpp/route_test.cc builds it alone and compares
// decide() with the rule it replaced, field by field).  crc32c_device.hip takes every such decision from decide(): the
// launch (launch_batch_body), the plan a checksum step inside a larger call needs (ensure_plan_for), and the two query
// entry points (kvsep_crc32c_plan_query, kvsep_crc32c_kernel_name) all read the one Route it returns.  Every measured
// crossover is written here and nowhere else; the choice never changes a result -- every kernel is exact for any block,
// whatever the hint.
#pragma once
#include <algorithm>
#include <cstdint>

#include "plan_size.h"

namespace kvsep {

constexpr int kWgThreads = 512;  // default CRC workgroup: 8 waves, 2 per SIMD (see launch_pieces_v)
static_assert(kWgThreads / 64 == kPlanWavesPerWg, "plan_size.h sizes plans for the default CRC workgroup");

constexpr uint64_t kNarrowMax = 32 * 1024;  // longest block the narrow kernel is ever chosen for (route::decide)
constexpr uint64_t kCoopMaxLen = 4096;  // crc32c_narrow_coop_kernel: 8 waves x 4 rows of 128 B; longer blocks go wide

// The combine kernel's grid (crc32c_support.inc): at most this many workgroups of 256 threads, a block per thread.
constexpr uint32_t kCombineMaxGrid = 2048;

// The claim kernel's shipped levers (crc32c_narrow_claim_kernel's kLean, round 6): the fill fetching each table entry
// once and no head / tail loads for groups without such chunks -- 16 of config 2's 52 non-payload loads per wave.  On
// one MI355X, interleaved in one process against the round-5 form (diag variant 65; tools/narrow_variants_probe.py,
// profiles/round6/claim_lean.log): 4 KiB blocks 128 MiB 24.66 vs 24.88 us, 256 MiB 43.93 vs 44.32, 1 GiB 153.98 vs
// 154.06 -- about 1 % at config 2, the time the loads cost; the rest of config 2's distance to the streaming read is not
// in instruction count.  Bit 2 (no init load for init-less batches) measured nothing and is not shipped.
constexpr uint32_t kClaimLean = 3;

namespace route {

// kvsep_crc32c_ctx_set_kernel's numbers (the C ABI takes them as an int; kvsep.KERNELS names them in Python).
enum class Kernel : int {
  Auto = 0,      // the measured crossovers below
  Wide = 1,      // crc32c_pieces_kernel only
  Narrow = 2,    // a narrow kernel whenever the hint allows one, its form by the crossovers
  Narrow16 = 3,  // the rest: that form, whenever the hint allows a narrow kernel
  Narrow8 = 4,
  Sorted = 5,
  Claim = 6,
  Claim16 = 7,
  Coop = 8,
};

// What a decision reads from a context.
struct Settings {
  int num_cus;
  uint64_t piece_bytes;
  bool piece_auto;  // smaller pieces for small batches (plan::piece_for); off once the size was set explicitly
  int dynamic;      // -1 auto, 0 static, 1 guided
  Kernel kernel;
};

// The kernel a batch runs on: the wide kernel, or one of the narrow forms for unsplit batches of short blocks.  The
// narrow forms keep the numbers they have had since they were variants of the tools build (KVSEP_NARROW, the tools and
// the profiles' READMEs name them so).
enum class Form : int {
  Wide = 0,       // crc32c_pieces_kernel
  Narrow16 = 6,   // crc32c_narrow_kernel, 16-wave workgroups
  Narrow8 = 9,    // crc32c_narrow_kernel, 8-wave workgroups (fill overlapped with the first loads)
  Claim = 10,     // crc32c_narrow_claim_kernel: workgroup-contiguous runs dealt by LDS claims, 8 waves
  Claim16 = 11,   // the same with 16-lane slots (4-block groups of Z_256 rows)
  Coop = 12,      // crc32c_narrow_coop_kernel: the workgroup's 8 waves on one group.  set_kernel only: measured 1.5x
                  // the claim kernel's time on config 2, see its header
  Sorted = 20,    // crc32c_narrow_sorted_kernel: sorted windows, 16 waves
};

inline const char* kernel_name(Form f) {
  switch (f) {
    case Form::Wide: return "crc32c_pieces_kernel";
    case Form::Sorted: return "crc32c_narrow_sorted_kernel";
    case Form::Claim:
    case Form::Claim16: return "crc32c_narrow_claim_kernel";
    case Form::Coop: return "crc32c_narrow_coop_kernel";
    default: return "crc32c_narrow_kernel";
  }
}

// KVSEP_DIAG tools build only: the KVSEP_NARROW value of a context, passed to decide() as a plain number (the shipped
// library passes none and reads no variable).  0: never a narrow kernel; 1 and 7: the shipped rule; a shipped form's
// number other than 12: that form; anything else: the variant of that number (crc32c_diag.inc) in place of the form --
// 12 is the variant there, and the coop form is reached by set_kernel alone.
constexpr int kDiagNone = 1;

// What a batch call runs as.
struct Route {
  bool planned;            // split into pieces through a plan, or every block one item
  plan::Piece piece;       // the piece size and its table (plan::piece_for; the context's own when unplanned)
  bool dyn;                // the guided schedule (one atomic per grab), or the static one
  Form form;
  uint64_t hint;           // PiecesArgs::hint of the narrow forms (0: the wide kernel takes none)
  unsigned threads;        // the CRC kernel's workgroup
  unsigned combine_grid;   // workgroups of the combine kernel that follows a planned batch (0: unplanned, none runs)
  uint64_t pieces_needed;  // plan entries the call needs (plan::pieces_needed; 0: unplanned)
  int variant;             // KVSEP_DIAG tools build only: the narrow variant that runs in place of `form` (kDiagNone)
};

inline Route decide(const Settings& s, uint64_t count, uint64_t total_bytes, uint64_t max_len, int diag = kDiagNone) {
  Route r;
  // split into pieces through a plan unless every block is known (from the max_len hint) to fit one piece
  r.planned = !(max_len != 0 && max_len <= s.piece_bytes);
  r.piece = r.planned ? plan::piece_for(s.piece_bytes, s.piece_auto, s.num_cus, total_bytes)
                      : plan::Piece{s.piece_bytes, -1};
  r.pieces_needed = r.planned ? plan::pieces_needed(r.piece.bytes, count, total_bytes) : 0;
  r.combine_grid = r.planned ? unsigned(std::min<uint64_t>((count + 255) / 256, kCombineMaxGrid)) : 0u;
  // auto schedule: guided (one atomic per grab) for planned batches with many pieces; static for the rest --
  // a few thousand small pieces would spend most of the kernel in single-item grabs on one counter
  // (~88 dequeues/us, MI355X_MICROARCH.md dequeue)
  const uint64_t est_items = r.planned ? count + total_bytes / r.piece.bytes : count;
  const uint64_t nwaves_est = uint64_t(s.num_cus) * (kWgThreads / 64);
  r.dyn = s.dynamic < 0 ? (r.planned && est_items >= 8 * nwaves_est) : s.dynamic == 1;
  r.form = Form::Wide;
  r.hint = 0;
  r.threads = kWgThreads;
  r.variant = kDiagNone;

  // A ragged batch: the max_len hint above 1.25x the mean length total_bytes / count (0 = unknown: not ragged).
  const bool ragged = count != 0 && total_bytes != 0 && 4 * max_len > 5 * (total_bytes / count);

  // The claim kernel with 16-lane slots (form 11: 4-block groups of Z_256 rows) for uniform blocks of 8-12 KiB, from 4 Ki
  // of them up to 512 MiB.  Its groups are half the bytes of the 8-lane form's, so the waves' last groups end closer
  // together.  Measured against the routing before it in one process (profiles/round4/claim_shapes/claim16*.log, graph
  // replay, two boxes): 8 KiB blocks 32 MiB 11.05 vs 11.70 us, 64 MiB 15.73 vs 16.81, 128 MiB 23.94 / 24.14 vs 25.49 /
  // 25.29, 256 MiB 41.73 / 42.08 vs 43.78 / 44.08, 512 MiB 80.43 / 80.45 vs 81.73 / 82.07 (1 GiB equal); 10 KiB 64 MiB
  // 14.15 vs 19.89, 128 MiB 24.85 vs 31.30, 256 MiB 44.76 vs 44.13, 512 MiB 80.48 vs 82.61; 12 KiB 64 MiB 15.84 vs
  // 17.48, 128 MiB 28.88 / 28.12 vs 29.51 / 30.17, 256 MiB 46.01 / 45.68 vs 52.99 / 53.16, 512 MiB 90.06 / 89.33 vs
  // 93.73 / 93.18.  Outside that box it loses: 2 KiB and 6-7 KiB blocks at most sizes, 14-32 KiB blocks, 1 GiB.
  const uint64_t bytes = total_bytes ? total_bytes : count * max_len;
  const bool claim16 = max_len >= 8 * 1024 && max_len <= 12 * 1024 && count >= 4096 && bytes <= (512ull << 20);

  // Narrow or wide kernel for an unsplit batch (every block <= piece_bytes, known from the max_len hint)?  The
  // narrow kernel's unit of parallelism is an 8-block group, so it needs many blocks; it wins on short blocks
  // when there are enough of them (measured, tools/ab_variants.py on one MI355X):
  //   <= 8 KiB blocks from 8 Ki blocks up (8 Ki x 4 KiB: 2.58 vs 2.13 TB/s; 4 Ki x 4 KiB: wide 1.50 vs 1.46),
  //   <= 16 KiB blocks from 16 Ki blocks up (16 Ki x 16 KiB: 5.58 vs 5.36; 4 Ki x 16 KiB: wide 3.67 vs 2.58),
  //   <= 32 KiB blocks from 32 Ki blocks up (32 Ki x 32 KiB: 6.72 vs 6.35; 16 Ki x 32 KiB: wide 6.12 vs 6.06),
  //   64 KiB blocks never (16 Ki x 64 KiB: wide 6.22 vs 4.88).
  // The thresholds scale with the CU count (256 on MI355X).  kvsep_crc32c_ctx_set_kernel can force either kernel
  // (tests).
  if (r.planned || max_len > 2 * kNarrowMax || s.kernel == Kernel::Wide) return r;
  if (s.kernel == Kernel::Auto) {
    const uint64_t cus = uint64_t(s.num_cus);
    const bool enough = (claim16 && !ragged) || (max_len <= 8 * 1024 && count >= 32 * cus) ||
                        (max_len <= 16 * 1024 && count >= 64 * cus) || (max_len <= kNarrowMax && count >= 128 * cus);
    if (diag == 0 || (diag < 2 && !enough)) return r;  // (KVSEP_NARROW: 0 never narrow, >= 2 always)
  }

  switch (s.kernel) {
    case Kernel::Narrow16: r.form = Form::Narrow16; break;
    case Kernel::Narrow8: r.form = Form::Narrow8; break;
    case Kernel::Sorted: r.form = Form::Sorted; break;
    case Kernel::Claim: r.form = Form::Claim; break;
    case Kernel::Claim16: r.form = Form::Claim16; break;
    case Kernel::Coop: r.form = Form::Coop; break;
    default:
      // 16-wave workgroups below 128 Ki blocks of <= 8 KiB (32 Ki blocks of 8-32 KiB), 8-wave ones from there on.  A
      // small batch gives each wave only a couple of 8-block groups, and more waves hide more of the launch/first-load
      // ramp (256 MiB of 4 KiB blocks: 16 waves +2-5 %); a large one streams better with 8 (1 GiB of 4 KiB blocks:
      // +5 %; 32 Ki x 16 KiB +2 %, 32 Ki x 32 KiB +6 %).  The 8-wave kernel overlaps the LDS fill with the first
      // group's loads (+0.3-2 %); at 16 waves that overlap measured -5 %.
      // Ragged batches take the sorted-window kernel at any size: an 8-block group waits for its longest block, and
      // sorting 64-block windows by length makes the groups even (config 4's 902 K blocks <= 32 KiB: 0.93 -> 0.57 ms
      // against the 16-wave narrow kernel, 1.24 ms on the 8-wave one).
      if (ragged) r.form = Form::Sorted;
      else if (claim16) r.form = Form::Claim16;
      // The claim kernel (crc32c_narrow_claim_kernel) for uniform blocks of <= 8 KiB from 32 Ki of them up to 384 Ki of
      // <= 4 KiB (128 MiB - 1.5 GiB of 4 KiB blocks) or 64 Ki of 4-8 KiB.  Measured against both forms below in one
      // process (profiles/round4/queue_variants/claim_*.log, graph replay): 4 KiB blocks 128 MiB 26.8 vs 27.8 us, 256 MiB
      // 45.9 vs 48.3, 512 MiB 83.1 vs 91.0, 1 GiB 156.7 vs 166.6, 1.5 GiB 241.4 vs 252.9, but 2 GiB 347.6 vs 314.0 (the
      // wave-major 8-wave kernel streams better from there); 2 KiB blocks 256 MiB 44.9 vs 47.6, 1 GiB 165.1 vs 163.8;
      // 8 KiB blocks 256 MiB 45.2 vs 45.8, 1 GiB 156.9 vs 155.0; 16 KiB blocks never (256 MiB 50.1 vs 44.0).
      else if (max_len <= 8 * 1024 && count >= (1u << 15) && count <= (max_len <= 4 * 1024 ? 3u << 17 : 1u << 16))
        r.form = Form::Claim;
      else if (max_len <= 8 * 1024 ? count >= (1u << 17) : count >= (1u << 15)) r.form = Form::Narrow8;
      else r.form = Form::Narrow16;
      if (diag != kDiagNone && diag != 7) {  // KVSEP_DIAG tools build only
        const bool shipped = diag == 6 || diag == 9 || diag == 10 || diag == 11 || diag == 20;
        r.form = shipped ? Form(diag) : Form::Narrow16;
        if (!shipped) r.variant = diag;
      }
  }
  r.hint = max_len;
  if (r.form == Form::Coop) r.hint = std::min(r.hint, kCoopMaxLen);  // its rows cover 4 KiB; longer blocks take its wide path
  if (r.form == Form::Narrow16 || r.form == Form::Sorted) r.threads = 1024;
  return r;
}

}  // namespace route
}  // namespace kvsep
