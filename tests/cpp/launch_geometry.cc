// launch_geometry.cc -- host only: the grid and block size of every kernel of a framing call, from the same pure
// headers the launch code takes them from, so that tests/test_isa_envelope_framing.py copies no formula.
//
//   launch_geometry constants
//   launch_geometry offsets  COUNT
//   launch_geometry verdicts COUNT
//   launch_geometry log      IMAGE_BYTES CAP
//   launch_geometry chains   CAP
//   launch_geometry logw     COUNT FRAG_CAP
//   launch_geometry concat   COUNT
//   launch_geometry pack     COUNT TARGET_WORKGROUPS   (also prints "short_wgs N" and "team N" for PackArgs)
//   launch_geometry scratch  offsets COUNT | log NBLOCKS | chains CAP
//
// One line per kernel, in stream order: "<kernel> <grid> <threads>"; a grid of 0 is a kernel the call does not launch.
// `constants` prints "<name> <value>" lines instead, and so does `scratch`: "words" an array sized for the argument
// holds, then the word offset of each slice a call over it takes -- what the launch code sizes and slices with.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chain_run.h"
#include "log_run.h"
#include "logw_run.h"
#include "offsets_run.h"
#include "pack_run.h"

using namespace kvsep;

static void line(const char* kernel, uint64_t grid, uint32_t threads) {
  std::printf("%s %" PRIu64 " %u\n", kernel, grid, threads);
}

static void offsets_pass(uint64_t count) {
  const uint64_t nt = offsets::tile_count(count);
  line("offsets_tile_sum_kernel", nt, offsets::kThreads);
  line("offsets_tile_scan_kernel", nt ? 1 : 0, offsets::kScanThreads);
  line("offsets_write_kernel", nt ? nt : 1, offsets::kThreads);  // an empty batch: the write kernel alone
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const auto arg = [&](int i) { return i < argc ? std::strtoull(argv[i], nullptr, 0) : 0ull; };
  const char* what = argv[1];
  if (!std::strcmp(what, "constants")) {
    std::printf("offsets_kTile %u\noffsets_kWaveLanes %u\noffsets_kScanThreads %u\n", offsets::kTile, offsets::kWaveLanes,
                offsets::kScanThreads);
    std::printf("list_kTile %u\nlist_kThreads %u\n", kListTile, kListThreads);
    std::printf("log_kBlock %" PRIu64 "\nlog_kHeader %" PRIu64 "\nlog_kThreads %u\n", logrun::kBlock, logrun::kHeader,
                logrun::kThreads);
    std::printf("chain_kTile %u\n", chain::kTile);
    std::printf("concat_kPerWg %" PRIu64 "\nconcat_kShortMax %" PRIu64 "\nconcat_kPassSegs %" PRIu64 "\n", concat::kPerWg,
                concat::kShortMax, concat::kPassSegs);
    std::printf("pack_kTile %" PRIu64 "\npack_kShortBlocks %u\npack_kChunkBlocks %u\n", pack::kTile, pack::kShortBlocks,
                pack::kChunkBlocks);
    std::printf("logw_kAhead %u\nlogw_kWaveLanes %u\nlogw_kBlock %u\nlogw_kAvail %u\nlogw_kFillThreads %u\n", logw::kAhead,
                logw::kWaveLanes, logw::kBlock, logw::kAvail, logw::kFillThreads);
  } else if (!std::strcmp(what, "scratch") && argc > 2 && !std::strcmp(argv[2], "offsets")) {
    const offsets::TileWords w = offsets::tile_words(offsets::tile_count(arg(3)));
    std::printf("words %" PRIu64 "\ntile_sum %" PRIu64 "\ntile_kept %" PRIu64 "\ntile_base %" PRIu64 "\ngrand %" PRIu64
                "\n", offsets::scratch_words(arg(3)), w.sum, w.kept, w.base, w.grand);
  } else if (!std::strcmp(what, "scratch") && argc > 2 && !std::strcmp(argv[2], "log")) {
    const logrun::Words w = logrun::words(arg(3));
    std::printf("words %" PRIu64 "\nstop %" PRIu64 "\ncnt %" PRIu64 "\nbase %" PRIu64 "\nfirst %" PRIu64 "\nstate %" PRIu64
                "\ncand %" PRIu64 "\ndrop %" PRIu64 "\nbadlen %" PRIu64 "\n", logrun::scratch_words(arg(3)), w.stop, w.cnt,
                w.base, w.first, w.state, w.cand, w.drop, w.badlen);
  } else if (!std::strcmp(what, "scratch") && argc > 2 && !std::strcmp(argv[2], "chains")) {
    const chain::TileWords w = chain::tile_words(chain::tile_count(arg(3)));
    std::printf("words %" PRIu64 "\nsum %" PRIu64 "\nin %" PRIu64 "\ngrand %" PRIu64 "\n", chain::scratch_words(arg(3)),
                w.sum, w.in, w.grand);
  } else if (!std::strcmp(what, "offsets")) {
    offsets_pass(arg(2));
  } else if (!std::strcmp(what, "verdicts")) {
    const uint64_t nt = list_tile_count(arg(2));
    line("verdict_tile_count_kernel", nt, kListThreads);
    line("verdict_tile_scan_kernel", nt ? 1 : 0, kListThreads);
    line("verdict_scatter_kernel", nt, kListThreads);
  } else if (!std::strcmp(what, "log")) {
    const uint64_t nb = logrun::block_count(arg(2)), cap = arg(3);
    line("log_count_kernel", nb ? logrun::grid_for(nb) : 0, logrun::kThreads);
    offsets_pass(nb);
    line("log_fill_kernel", logrun::pad_grid(nb, cap), logrun::kThreads);
    line("log_block_kernel", nb ? logrun::grid_for(nb) : 0, logrun::kThreads);
    line("log_stop_kernel", logrun::kReduceGrid, logrun::kThreads);
    line("log_accept_kernel", logrun::pad_grid(nb, cap), logrun::kThreads);
    line("log_totals_kernel", logrun::kReduceGrid, logrun::kThreads);
  } else if (!std::strcmp(what, "chains")) {
    const uint64_t cap = arg(2), nt = chain::tile_count(cap);
    line("chain_tile_kernel", nt, chain::kThreads);
    line("chain_scan_kernel", nt ? 1 : 0, chain::kScanThreads);
    line("chain_write_kernel", chain::write_tiles(cap), chain::kThreads);
    line("chain_reclen_kernel", chain::reclen_grid(cap), chain::kThreads);
  } else if (!std::strcmp(what, "logw")) {
    const uint64_t lanes = logw::fill_lanes(arg(2), arg(3));
    line("logw_layout_kernel", 1, logw::kLayoutThreads);
    line("logw_fill_kernel", (lanes + logw::kFillThreads - 1) / logw::kFillThreads, logw::kFillThreads);
  } else if (!std::strcmp(what, "concat")) {
    line("crc32c_concat_kernel", concat::grid_for(arg(2)), kConcatThreads);
  } else if (!std::strcmp(what, "pack")) {  // TARGET_WORKGROUPS: what the launch code derives from the CU count
    const uint32_t team = pack::team_size(arg(2), uint32_t(arg(3)));
    line("crc32c_pack_kernel", arg(2) ? pack::short_wgs(arg(2)) + pack::chunk_count(arg(2)) * team : 0, kPackThreads);
    std::printf("short_wgs %u\nteam %u\n", pack::short_wgs(arg(2)), team);
  } else {
    return 2;
  }
  return 0;
}
