// sstw_geometry.cc -- host only: the grid and block size of every kernel of an SST table-writer call and the slices of
// its scratch, from the same pure headers the launch code takes them from (sstw_run.h, sst_run.h, offsets_run.h), so
// that tests/test_isa_envelope_sstw.py copies no formula.
//
//   sstw_geometry constants
//   sstw_geometry scratch COUNT     the builder's scratch for COUNT entries: its words and the word offset of each slice
//   sstw_geometry build COUNT       kvsep_sst_index_build_device / kvsep_sst_table_finish_device without the CRC call:
//                                   size, the offsets pass twice, fill, tail
//   sstw_geometry keys RUNS CAP     kvsep_sst_index_keys_device: keys count, stop, the offsets pass over RUNS, keys fill
//   sstw_geometry keep CAP          the rewrite's keep-mask kernel
//
// One line per kernel, in stream order: "<kernel> <grid> <threads>"; the other forms print "<name> <value>" lines.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "offsets_run.h"
#include "sst_run.h"
#include "sstw_run.h"

using namespace kvsep;

static void line(const char* kernel, uint64_t grid, uint32_t threads) {
  std::printf("%s %" PRIu64 " %u\n", kernel, grid, threads);
}

static void offsets_pass(uint64_t count) {
  const uint64_t nt = offsets::tile_count(count);
  line("offsets_tile_sum_kernel", nt, offsets::kThreads);
  line("offsets_tile_scan_kernel", nt ? 1 : 0, offsets::kScanThreads);
  line("offsets_write_kernel", nt ? nt : 1, offsets::kThreads);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const auto arg = [&](int i) { return i < argc ? std::strtoull(argv[i], nullptr, 0) : 0ull; };
  const char* what = argv[1];
  if (!std::strcmp(what, "constants")) {
    std::printf("kStageBytes %u\nkTrailer %" PRIu64 "\nkFooter %" PRIu64 "\nkMetaFramed %" PRIu64 "\nkEmptyBlock %" PRIu64
                "\nkStopWords %" PRIu64 "\n",
                sstw::kStageBytes, sstw::kTrailer, sstw::kFooter, sstw::kMetaFramed, sstw::kEmptyBlock, sst::kStopWords);
    std::printf("kEntriesBytes %d\nkNKept %d\nkCrcOff %d\nkCrcLen %d\nkCrc %d\nkWords %d\n", int(sstw::kEntriesBytes),
                int(sstw::kNKept), int(sstw::kCrcOff), int(sstw::kCrcLen), int(sstw::kCrc), int(sstw::kWords));
  } else if (!std::strcmp(what, "scratch")) {
    const sstw::Slices s = sstw::slices(arg(2));
    const offsets::TileWords w = offsets::tile_words(offsets::tile_count(arg(2)));
    std::printf("total %" PRIu64 "\nsize %" PRIu64 "\nflag %" PRIu64 "\npos %" PRIu64 "\nrank %" PRIu64 "\nkeep %" PRIu64
                "\nwords %" PRIu64 "\n",
                sstw::scratch_words(arg(2)), s.size, s.flag, s.pos, s.rank, s.keep, s.words);
    std::printf("tile_words %" PRIu64 "\ntile_sum %" PRIu64 "\ntile_kept %" PRIu64 "\ntile_base %" PRIu64 "\ngrand %" PRIu64
                "\n", offsets::scratch_words(arg(2)), w.sum, w.kept, w.base, w.grand);
  } else if (!std::strcmp(what, "walk_scratch")) {  // RUNS: as sst_geometry's scratch
    const offsets::TileWords w = offsets::tile_words(offsets::tile_count(arg(2)));
    std::printf("words %" PRIu64 "\nworkgroups %" PRIu64 "\ntiles %" PRIu64 "\n", sst::scratch_words(arg(2)),
                sst::grid_for(arg(2)), offsets::tile_count(arg(2)));
    std::printf("tile_words %" PRIu64 "\ntile_sum %" PRIu64 "\ntile_kept %" PRIu64 "\ntile_base %" PRIu64 "\ngrand %" PRIu64
                "\n", offsets::scratch_words(arg(2)), w.sum, w.kept, w.base, w.grand);
  } else if (!std::strcmp(what, "build")) {
    if (arg(2)) line("sstw_size_kernel", sstw::grid_for(arg(2)), sstw::kThreads);
    offsets_pass(arg(2));
    offsets_pass(arg(2));
    line("sstw_fill_kernel", sstw::grid_for(arg(2)), sstw::kThreads);
    line("sstw_tail_kernel", 1, sstw::kTailThreads);
  } else if (!std::strcmp(what, "keys")) {
    line("sst_keys_count_kernel", sst::grid_for(arg(2)), sst::kThreads);
    line("sst_index_stop_kernel", 1, sst::kThreads);
    offsets_pass(arg(2));
    line("sst_keys_fill_kernel", sst::pad_grid(arg(2), arg(3)), sst::kThreads);
  } else if (!std::strcmp(what, "keep")) {
    line("sstw_keep_kernel", sstw::grid_for(arg(2)), sstw::kThreads);
  } else {
    return 2;
  }
  return 0;
}
