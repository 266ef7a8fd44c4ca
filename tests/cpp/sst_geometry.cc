// sst_geometry.cc -- host only: the grid and block size of every kernel of an SST table-reader call and the size of
// its scratch, from the same pure headers the launch code takes them from (sst_run.h, offsets_run.h), so that
// tests/test_isa_envelope_sst.py copies no formula.
//
//   sst_geometry constants
//   sst_geometry walk  RUNS CAP     kvsep_sst_index_device: count, stop, the offsets pass over RUNS, fill
//   sst_geometry table RUNS CAP     kvsep_sst_table_verify_device without its CRC calls: footer, prep of one slot, the
//                                   walk, prep of CAP slots
//
// One line per kernel, in stream order: "<kernel> <grid> <threads>".  `constants` prints "<name> <value>" lines instead.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "offsets_run.h"
#include "sst_run.h"

using namespace kvsep;

static void line(const char* kernel, uint64_t grid, uint32_t threads) {
  std::printf("%s %" PRIu64 " %u\n", kernel, grid, threads);
}

static void walk(uint64_t runs, uint64_t cap) {
  const uint64_t nt = offsets::tile_count(runs);
  line("sst_index_count_kernel", sst::grid_for(runs), sst::kThreads);
  line("sst_index_stop_kernel", 1, sst::kThreads);
  line("offsets_tile_sum_kernel", nt, offsets::kThreads);
  line("offsets_tile_scan_kernel", nt ? 1 : 0, offsets::kScanThreads);
  line("offsets_write_kernel", nt ? nt : 1, offsets::kThreads);
  line("sst_index_fill_kernel", sst::pad_grid(runs, cap), sst::kThreads);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const auto arg = [&](int i) { return i < argc ? std::strtoull(argv[i], nullptr, 0) : 0ull; };
  const char* what = argv[1];
  if (!std::strcmp(what, "constants")) {
    std::printf("kThreads %u\nkStopWords %" PRIu64 "\nkMaskOfZero %u\nkNoMatch %u\nkFooter %" PRIu64 "\n", sst::kThreads,
                sst::kStopWords, sst::kMaskOfZero, sst::kNoMatch, sst::kFooter);
    std::printf("offsets_kTile %u\n", offsets::kTile);
  } else if (!std::strcmp(what, "scratch")) {  // RUNS: words of the walk's scratch, workgroups of its count kernel,
    // then the offsets pass over the runs: its tiles, its tile words and the word offset of each slice of them
    const offsets::TileWords w = offsets::tile_words(offsets::tile_count(arg(2)));
    std::printf("words %" PRIu64 "\nworkgroups %" PRIu64 "\ntiles %" PRIu64 "\n", sst::scratch_words(arg(2)),
                sst::grid_for(arg(2)), offsets::tile_count(arg(2)));
    std::printf("tile_words %" PRIu64 "\ntile_sum %" PRIu64 "\ntile_kept %" PRIu64 "\ntile_base %" PRIu64 "\ngrand %" PRIu64
                "\n", offsets::scratch_words(arg(2)), w.sum, w.kept, w.base, w.grand);
  } else if (!std::strcmp(what, "walk")) {
    walk(arg(2), arg(3));
  } else if (!std::strcmp(what, "table")) {
    line("sst_footer_kernel", 1, sst::kFooterThreads);
    line("sst_table_prep_kernel", 1, sst::kThreads);
    walk(arg(2), arg(3));
    line("sst_table_prep_kernel", sst::grid_for(arg(3)), sst::kThreads);
  } else {
    return 2;
  }
  return 0;
}
