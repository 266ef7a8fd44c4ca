// framing.cpp -- the record/block framings that call crc32c in kv-separate, batched onto the engine.
//
//   vlog       db/value_log_writer.cc:46-76, db/value_log_reader.cc:86-138, db/log_format.h:40
//              record = [Mask(Value(payload)) LE32][len LE32][payload]; the reader stops at the first
//              truncated record (eof) and at the first checksum mismatch (ReportCorruption + eof_).
//   log/MANIFEST db/log_writer.cc:84-115, db/log_reader.cc:189-272, db/log_format.h:16-33
//              32 KiB blocks of [crc LE32][len LE16][type u8][payload]; crc = Mask(Value(type||payload));
//              < 7 trailing bytes of a block are padding; type 0 with length 0 is preallocated space.
//   SST block  table/table_builder.cc:209-232, table/format.cc:73-108, table/format.h:81
//              block, then a 5-byte trailer [type u8][Mask(Extend(Value(block), &type, 1)) LE32].
//
// The serial parts (header walks) stay on the host; every checksum goes through one batched call.
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/kvsep_crc32c.h"
#include "chain_run.h"
#include "logw_run.h"
#include "sst_run.h"
#include "sstw_run.h"

namespace kvsep {
// crc32c_host.cpp: copies dst[i] <- src[i] (n[i] bytes) on the context's copier threads.
int host_copy_parallel(kvsep_crc32c_ctx* c, char* const* dst, const char* const* src, const uint64_t* n,
                       uint64_t count);
// crc32c_host.cpp: kvsep_crc32c_batch_host whose gather also copies record i to tee[i] (one read of each payload).
int batch_host_tee(kvsep_crc32c_ctx* c, const uint32_t* init, const char* const* ptr, const uint64_t* len,
                   uint32_t* out, uint64_t count, char* const* tee);
void set_last_error(const char* msg);  // crc32c_host.cpp: the message kvsep_last_error() returns
}  // namespace kvsep

namespace {

inline uint32_t le32(const char* p) {
  const auto* b = reinterpret_cast<const uint8_t*>(p);
  return uint32_t(b[0]) | (uint32_t(b[1]) << 8) | (uint32_t(b[2]) << 16) | (uint32_t(b[3]) << 24);
}

inline void put_le32(char* p, uint32_t v) {
  auto* b = reinterpret_cast<uint8_t*>(p);
  b[0] = uint8_t(v);
  b[1] = uint8_t(v >> 8);
  b[2] = uint8_t(v >> 16);
  b[3] = uint8_t(v >> 24);
}

constexpr uint64_t kVlogHeader = 8;       // db/log_format.h:40
constexpr uint64_t kLogBlock = 32768;     // db/log_format.h:30
constexpr uint64_t kLogHeader = 7;        // db/log_format.h:33
constexpr uint64_t kSstTrailer = 5;       // table/format.h:81 kBlockTrailerSize
constexpr uint8_t kLogEofCode = 5;        // db/log_reader.h:66,72: kEof = kMaxRecordType + 1, kBadRecord = + 2 share
constexpr uint8_t kLogBadRecordCode = 6;  // the value space of the type byte ReadPhysicalRecord returns

// Every invalid-argument return posts its reason first, so kvsep_last_error() never carries a stale message.
inline int einval(const char* why) {
  kvsep::set_last_error(why);
  return KVSEP_EINVAL;
}

// One pass over a log image the way ReadPhysicalRecord (db/log_reader.cc:189-272) parses it: rec(p, l, t) for every
// physical record whose header at p fits its block, skip(p, end, zero) where the reader drops the rest [p, end) of a
// block without looking at a checksum -- a length past the block end (:224-235, zero = false) or a preallocated zero
// header (:237-243, zero = true).  Both are kBadRecord to ReadRecord, unless the block is the short last one.
template <class Rec, class Skip>
inline void log_scan(const char* buf, uint64_t n, Rec rec, Skip skip) {
  for (uint64_t blk = 0; blk < n; blk += kLogBlock) {
    const uint64_t end = blk + kLogBlock < n ? blk + kLogBlock : n;
    uint64_t p = blk;
    while (end - p >= kLogHeader) {  // :192-215: < 7 bytes left = block trailer
      const uint8_t* h = reinterpret_cast<const uint8_t*>(buf + p);
      const uint64_t l = uint64_t(h[4]) | (uint64_t(h[5]) << 8);
      const uint8_t t = h[6];
      if (kLogHeader + l > end - p) {  // bad record length: drop rest of block
        skip(p, end, false);
        break;
      }
      if (t == 0 && l == 0) {  // preallocated zero region
        skip(p, end, true);
        break;
      }
      rec(p, l, t);
      p += kLogHeader + l;
    }
  }
}

}  // namespace

extern "C" {

uint64_t kvsep_vlog_walk(const char* buf, uint64_t n, uint64_t* off, uint64_t* len, uint32_t* stored,
                         uint64_t cap, uint64_t* consumed) {
  uint64_t p = 0, k = 0;
  while (p + kVlogHeader <= n) {  // db/value_log_reader.cc:91-96: short header = eof
    const uint64_t l = le32(buf + p + 4);
    if (l > n - p - kVlogHeader) break;  // :107-108: short payload = eof
    if (k < cap) {
      if (off) off[k] = p + kVlogHeader;
      if (len) len[k] = l;
      if (stored) stored[k] = le32(buf + p);
    }
    ++k;
    p += kVlogHeader + l;
  }
  if (consumed) *consumed = p;
  return k;
}

int kvsep_vlog_verify_host(kvsep_crc32c_ctx* ctx, const char* buf, uint64_t n, uint64_t* nrecords, uint64_t* ngood,
                           uint64_t* good_bytes, uint64_t* drop_bytes) {
  if (!ctx || (!buf && n)) return einval("kvsep_vlog_verify_host: null argument");
  const uint64_t cnt = kvsep_vlog_walk(buf, n, nullptr, nullptr, nullptr, 0, nullptr);
  std::vector<uint64_t> off(cnt), len(cnt);
  std::vector<uint32_t> stored(cnt), crc(cnt);
  kvsep_vlog_walk(buf, n, off.data(), len.data(), stored.data(), cnt, nullptr);
  if (cnt) {
    const int rc = kvsep_crc32c_batch_host_span(ctx, buf, n, off.data(), len.data(), nullptr, crc.data(), cnt);
    if (rc) return rc;
  }
  uint64_t g = 0;
  while (g < cnt && kvsep_crc32c_mask(crc[g]) == stored[g]) ++g;  // :109-122: stop at first mismatch
  if (nrecords) *nrecords = cnt;
  if (ngood) *ngood = g;
  if (good_bytes) *good_bytes = g ? off[g - 1] + len[g - 1] : 0;
  if (drop_bytes) *drop_bytes = g < cnt ? len[g] : 0;  // drop_size = buffer_.size() = the payload (:117-120)
  return KVSEP_OK;
}

int kvsep_vlog_frame_host(kvsep_crc32c_ctx* ctx, const char* const* payload, const uint64_t* len, uint64_t count,
                          char* dst, uint64_t dst_cap, uint64_t* written) {
  if (!ctx || (count && (!payload || !len))) return einval("kvsep_vlog_frame_host: null argument");
  uint64_t need = 0;
  for (uint64_t i = 0; i < count; ++i) {
    if (len[i] > 0xffffffffull)  // db/value_log_writer.cc:48 (LE32 length)
      return einval("kvsep_vlog_frame_host: payload longer than 2^32 - 1 bytes");
    need += kVlogHeader + len[i];
  }
  if (written) *written = need;
  if (need > dst_cap || (need && !dst)) return einval("kvsep_vlog_frame_host: destination too small");
  // Checksums first, then the payload copy into the framed image as a pass of its own.  For ~1 MiB group-commit
  // payloads that measured faster than copying each payload into the image from the gather that stages it (the
  // tee that the log writer's <= 32 KiB fragments use): 36.5 vs 31.3 GiB/s, medians of three alternating runs.
  std::vector<uint32_t> crc(count);
  if (count) {
    const int rc = kvsep_crc32c_batch_host(ctx, nullptr, payload, len, crc.data(), count);
    if (rc) return rc;
  }
  uint64_t p = 0;
  std::vector<char*> at(count);
  for (uint64_t i = 0; i < count; ++i) {  // db/value_log_writer.cc:57-70: [masked crc LE32][len LE32]
    put_le32(dst + p, kvsep_crc32c_mask(crc[i]));
    put_le32(dst + p + 4, uint32_t(len[i]));
    at[i] = dst + p + kVlogHeader;
    p += kVlogHeader + len[i];
  }
  return kvsep::host_copy_parallel(ctx, at.data(), payload, len, count);  // the payload bytes
}

int kvsep_vlog_frame_offsets(const uint64_t* len, uint64_t count, uint64_t start, uint64_t* rec_off, uint64_t* end) {
  if (count && (!len || !rec_off)) return einval("kvsep_vlog_frame_offsets: null argument");
  uint64_t p = start;
  for (uint64_t i = 0; i < count; ++i) {
    if (len[i] > 0xffffffffull)  // db/value_log_writer.cc:48 (LE32 length)
      return einval("kvsep_vlog_frame_offsets: payload longer than 2^32 - 1 bytes");
    rec_off[i] = p;
    const uint64_t rec = kVlogHeader + len[i];
    if (p + rec < p) return einval("kvsep_vlog_frame_offsets: the offsets leave 64 bits");
    p += rec;
  }
  if (end) *end = p;
  return KVSEP_OK;
}

uint64_t kvsep_log_walk(const char* buf, uint64_t n, uint64_t* off, uint64_t* len, uint32_t* stored, uint8_t* type,
                        uint64_t cap) {
  uint64_t k = 0;
  log_scan(
      buf, n,
      [&](uint64_t p, uint64_t l, uint8_t t) {
        if (k < cap) {
          if (off) off[k] = p + 6;  // CRC covers type || payload (:247-248)
          if (len) len[k] = 1 + l;
          if (stored) stored[k] = le32(buf + p);
          if (type) type[k] = t;
        }
        ++k;
      },
      [](uint64_t, uint64_t, bool) {});
  return k;
}

int kvsep_log_verify_host(kvsep_crc32c_ctx* ctx, const char* buf, uint64_t n, uint8_t* ok, uint64_t cap,
                          uint64_t* nrecords) {
  if (!ctx || (!buf && n)) return einval("kvsep_log_verify_host: null argument");
  const uint64_t cnt = kvsep_log_walk(buf, n, nullptr, nullptr, nullptr, nullptr, 0);
  if (nrecords) *nrecords = cnt;
  if (cnt > cap || (cnt && !ok)) return einval("kvsep_log_verify_host: verdict array too small");
  std::vector<uint64_t> off(cnt), len(cnt);
  std::vector<uint32_t> stored(cnt), crc(cnt);
  kvsep_log_walk(buf, n, off.data(), len.data(), stored.data(), nullptr, cnt);
  if (cnt) {
    const int rc = kvsep_crc32c_batch_host_span(ctx, buf, n, off.data(), len.data(), nullptr, crc.data(), cnt);
    if (rc) return rc;
  }
  for (uint64_t i = 0; i < cnt; ++i) ok[i] = crc[i] == kvsep_crc32c_unmask(stored[i]) ? 1 : 0;  // :250-258
  return KVSEP_OK;
}

int kvsep_log_frame_host(kvsep_crc32c_ctx* ctx, const char* const* payload, const uint64_t* len, uint64_t count,
                         uint64_t dest_length, char* dst, uint64_t dst_cap, uint64_t* written) {
  if (!ctx || (count && (!payload || !len))) return einval("kvsep_log_frame_host: null argument");
  struct Frag {
    const char* src;
    uint64_t len, at;  // payload bytes; offset of its header in dst
    uint8_t type;
  };
  std::vector<Frag> frags;
  std::vector<std::pair<uint64_t, uint64_t>> trailers;  // zero-filled block ends [at, at + n)
  uint64_t block_offset = dest_length % kLogBlock, p = 0;
  for (uint64_t r = 0; r < count; ++r) {  // log::Writer::AddRecord (:35-82)
    const char* ptr = payload[r];
    uint64_t left = len[r];
    bool begin = true;
    do {
      const uint64_t leftover = kLogBlock - block_offset;
      if (leftover < kLogHeader) {  // trailer: zero-filled, next block (:48-57)
        if (leftover) trailers.emplace_back(p, leftover);
        p += leftover;
        block_offset = 0;
      }
      const uint64_t avail = kLogBlock - block_offset - kLogHeader;
      const uint64_t frag = left < avail ? left : avail;
      const bool end = left == frag;
      const uint8_t type = begin && end ? 1 : begin ? 2 : end ? 4 : 3;  // FULL / FIRST / LAST / MIDDLE
      frags.push_back({ptr, frag, p, type});
      p += kLogHeader + frag;
      block_offset += kLogHeader + frag;
      ptr += frag;
      left -= frag;
      begin = false;
    } while (left > 0);
  }
  if (written) *written = p;
  if (p > dst_cap || (p && !dst)) return einval("kvsep_log_frame_host: destination too small");
  const uint64_t nf = frags.size();
  std::vector<const char*> src(nf);
  std::vector<uint64_t> flen(nf);
  std::vector<uint32_t> init(nf), crc(nf);
  uint32_t type_crc[5];
  for (int t = 0; t < 5; ++t) {  // InitTypeCrc (:16-21)
    const char c = char(t);
    type_crc[t] = kvsep_crc32c_extend_host(0, &c, 1);
  }
  for (uint64_t i = 0; i < nf; ++i) {
    src[i] = frags[i].src;
    flen[i] = frags[i].len;
    init[i] = type_crc[frags[i].type];
  }
  // the fragment bytes land in dst from the same gather that stages them for the checksum (a tee: one read each;
  // 36.0 vs 24.1 GiB/s against a second copy pass, medians of three alternating runs on one box)
  std::vector<char*> at(nf);
  for (uint64_t i = 0; i < nf; ++i) at[i] = dst + frags[i].at + kLogHeader;
  if (nf) {
    const int rc = kvsep::batch_host_tee(ctx, init.data(), src.data(), flen.data(), crc.data(), nf, at.data());
    if (rc) return rc;
  }
  for (const auto& t : trailers) std::memset(dst + t.first, 0, t.second);
  for (uint64_t i = 0; i < nf; ++i) {  // EmitPhysicalRecord (:84-115)
    char* h = dst + frags[i].at;
    put_le32(h, kvsep_crc32c_mask(crc[i]));
    h[4] = char(frags[i].len & 0xff);
    h[5] = char(frags[i].len >> 8);
    h[6] = char(frags[i].type);
  }
  return KVSEP_OK;
}

int kvsep_log_frame_layout(const uint64_t* len, const uint8_t* keep, uint64_t count, uint64_t dest_length,
                           uint64_t* rec_at, uint64_t* frag_first, uint64_t* nfrag, uint64_t* written) {
  namespace logw = kvsep::logw;
  if (!frag_first || (count && (!len || !rec_at))) return einval("kvsep_log_frame_layout: null argument");
  const uint32_t b0 = logw::start_state(dest_length);
  uint32_t raw = b0;               // the writer's offset behind the records so far (logw_run.h holds every rule)
  uint64_t block = 0, total = 0;   // blocks advanced, fragments
  for (uint64_t i = 0; i < count; ++i) {
    const bool kept = !keep || keep[i] != 0;
    frag_first[i] = total;
    const uint32_t b = logw::start_of(raw);
    const uint64_t nf = kept ? logw::nfrag(b, len[i]) : 0;
    block = logw::add_sat(block, kept ? logw::blocks_advanced(logw::resets(raw), nf) : 0);
    raw = logw::raw_behind(raw, kept, logw::step_of(kept, len[i]));
    const bool is_laid = logw::laid(kept, block, raw);
    rec_at[i] = logw::rec_at(is_laid, block, nf, b, b0);
    total = logw::add_sat(total, logw::frags_of(is_laid, nf));
  }
  frag_first[count] = total;
  if (nfrag) *nfrag = total;
  if (written) *written = logw::rel(logw::pos_sat(block, raw), b0);
  return KVSEP_OK;
}

int kvsep_sst_trailers_host(kvsep_crc32c_ctx* ctx, const char* const* block, const uint64_t* len, const uint8_t* types,
                            uint32_t* masked_out, uint64_t count) {
  if (!ctx || (count && (!block || !len || !types || !masked_out)))
    return einval("kvsep_sst_trailers_host: null argument");
  if (!count) return KVSEP_OK;
  // Value(block) for every block in one batched call through the pinned staging, then the trailer's one-byte
  // extension by the type and Mask on the host (table/table_builder.cc:222-225)
  const int rc = kvsep_crc32c_batch_host(ctx, nullptr, block, len, masked_out, count);
  if (rc) return rc;
  for (uint64_t i = 0; i < count; ++i) {
    const char t = char(types[i]);
    masked_out[i] = kvsep_crc32c_mask(kvsep_crc32c_extend_host(masked_out[i], &t, 1));
  }
  return KVSEP_OK;
}

int kvsep_sst_verify_host(kvsep_crc32c_ctx* ctx, const char* file, uint64_t n, const uint64_t* off, const uint64_t* len,
                          uint32_t* out, uint64_t* first_bad, uint64_t* nbad, uint64_t count) {
  if (!ctx || (!file && n) || (count && (!off || !len || !out))) return einval("kvsep_sst_verify_host: null argument");
  std::vector<uint64_t> len1(count);
  for (uint64_t i = 0; i < count; ++i) {
    // the handle must leave room for the 5-byte trailer (table/format.cc:84-87: "truncated block read")
    if (off[i] > n || len[i] > n - off[i] || n - off[i] - len[i] < kSstTrailer)
      return einval("kvsep_sst_verify_host: block handle (plus its 5-byte trailer) outside the file image");
    len1[i] = len[i] + 1;  // Value(data, n + 1): the block and its type byte (format.cc:102)
  }
  if (count) {
    const int rc = kvsep_crc32c_batch_host_span(ctx, file, n, off, len1.data(), nullptr, out, count);
    if (rc) return rc;
  }
  uint64_t fb = ~0ull, nb = 0;
  for (uint64_t i = 0; i < count; ++i) {
    if (out[i] != kvsep_crc32c_unmask(le32(file + off[i] + len[i] + 1))) {  // format.cc:101-106
      if (fb == ~0ull) fb = i;
      ++nb;
    }
  }
  if (first_bad) *first_bad = fb;
  if (nbad) *nbad = nb;
  return KVSEP_OK;
}

int kvsep_sst_footer(const char* file, uint64_t n, uint64_t handles[4], uint32_t* status) {
  if ((!file && n) || !handles || !status) return einval("kvsep_sst_footer: null argument");
  const auto rd = [file](uint64_t p) { return uint8_t(file[p]); };
  const kvsep::sst::Footer f = kvsep::sst::footer(rd, n);  // sst_run.h holds every rule
  for (int k = 0; k < 4; ++k) handles[k] = f.h[k];
  *status = f.status;
  return KVSEP_OK;
}

int kvsep_sst_index_walk(const char* blk, uint64_t blk_len, uint64_t* off, uint64_t* len, uint64_t cap,
                         uint64_t* nblocks, uint32_t* status) {
  namespace sst = kvsep::sst;
  if ((!blk && blk_len) || (cap && (!off || !len)) || !nblocks || !status)
    return einval("kvsep_sst_index_walk: null argument");
  const auto rd = [blk](uint64_t p) { return uint8_t(blk[p]); };
  uint64_t total = 0;
  uint32_t code = sst::kOk;
  const sst::Tail t = sst::tail(rd, 0, blk_len);
  if (!t.ok) code = sst::kBadRestarts;
  for (uint64_t r = 0; !code && r < t.nrestarts; ++r) {  // the runs in order: the first error is the lowest run's
    const sst::Run run = sst::run_of(rd, 0, t, r);
    if (!run.ok) {
      code = sst::kBadRestarts;
      break;
    }
    const sst::Walked w = sst::walk_run(rd, 0, run, t.restart_offset, [&](uint64_t k, uint64_t o, uint64_t l) {
      if (total + k < cap) off[total + k] = o, len[total + k] = l;
      return true;
    });
    total += w.count;
    code = w.status;
  }
  for (uint64_t i = sst::held(total, cap); i < cap; ++i) off[i] = len[i] = 0;
  *nblocks = total;
  *status = code;
  return KVSEP_OK;
}

int kvsep_sst_index_keys(const char* blk, uint64_t blk_len, uint64_t* off, uint64_t* len, uint64_t* key_off,
                         uint64_t* key_len, uint64_t cap, uint64_t* nblocks, uint32_t* status) {
  namespace sst = kvsep::sst;
  if ((!blk && blk_len) || (cap && (!off || !len || !key_off || !key_len)) || !nblocks || !status)
    return einval("kvsep_sst_index_keys: null argument");
  const auto rd = [blk](uint64_t p) { return uint8_t(blk[p]); };
  uint64_t total = 0;
  uint32_t code = sst::kOk;
  const sst::Tail t = sst::tail(rd, 0, blk_len);
  if (!t.ok) code = sst::kBadRestarts;
  for (uint64_t r = 0; !code && r < t.nrestarts; ++r) {  // the runs in order: the first error is the lowest run's
    const sst::Run run = sst::run_of(rd, 0, t, r);
    if (!run.ok) {
      code = sst::kBadRestarts;
      break;
    }
    const sst::Walked w = sst::walk_run_keys(
        rd, 0, run, t.restart_offset, [&](uint64_t k, uint64_t o, uint64_t l, uint64_t kat, uint64_t klen) {
          const uint64_t i = total + k;
          if (i < cap) off[i] = o, len[i] = l, key_off[i] = kat, key_len[i] = klen;
          return true;
        });
    total += w.count;
    code = w.status;
  }
  for (uint64_t i = sst::held(total, cap); i < cap; ++i) off[i] = len[i] = key_off[i] = key_len[i] = 0;
  *nblocks = total;
  *status = code;
  return KVSEP_OK;
}

int kvsep_sst_index_build(const char* key_base, const uint64_t* key_off, const uint64_t* key_len,
                          const uint64_t* blk_off, const uint64_t* blk_len, const uint8_t* keep, uint64_t count,
                          char* dst, uint64_t dst_bytes, uint64_t at, uint64_t* out_len, uint32_t* status) {
  namespace sstw = kvsep::sstw;
  if ((count && (!key_off || !key_len || !blk_off || !blk_len)) || !dst || !out_len || !status)
    return einval("kvsep_sst_index_build: null argument");
  if (count > 0xffffffffull) return einval("kvsep_sst_index_build: more than 2^32 - 1 entries");
  const auto kept = [&](uint64_t i) { return sstw::kept(keep ? keep[i] : uint8_t(1), blk_off[i]); };
  uint64_t entries = 0, nkept = 0;
  for (uint64_t i = 0; i < count; ++i) {  // the totals first: a refusal writes nothing
    entries = sstw::add_sat(entries, sstw::entry_size(kept(i), key_len[i], blk_off[i], blk_len[i]));
    nkept += kept(i);
  }
  const sstw::Plan p = sstw::plan(entries, nkept, at, 0, 0, dst_bytes, 0);
  *out_len = p.need;
  *status = p.status;
  if (p.status) return KVSEP_OK;
  char* blk = dst + p.at;
  uint64_t pos = 0, rank = 0;
  for (uint64_t i = 0; i < count; ++i) {
    if (!kept(i)) continue;
    const uint64_t kl = key_len[i], size = sstw::entry_size(true, kl, blk_off[i], blk_len[i]);
    const uint32_t h = sstw::head_len(kl);
    for (uint64_t j = 0; j < size; ++j)
      if (j < h || j >= h + kl) blk[pos + j] = char(sstw::frame_byte(j, kl, blk_off[i], blk_len[i]));
    if (kl) memcpy(blk + pos + h, key_base + key_off[i], kl);
    put_le32(blk + sstw::restart_at(entries, rank, i), uint32_t(pos));
    pos += size;
    ++rank;
  }
  if (sstw::lone_restart(nkept)) put_le32(blk + entries, 0);
  put_le32(blk + sstw::count_at(entries, nkept), sstw::count_word(nkept));
  const char type = 0;
  const uint32_t masked = kvsep_crc32c_mask(kvsep_crc32c_extend_host(kvsep_crc32c_extend_host(0, blk, p.len), &type, 1));
  for (uint32_t j = 0; j < sstw::kTrailer; ++j) blk[p.len + j] = char(sstw::trailer_byte(j, masked));
  return KVSEP_OK;
}

int kvsep_sst_footer_build(uint64_t meta_off, uint64_t meta_len, uint64_t index_off, uint64_t index_len, char out[48]) {
  if (!out) return einval("kvsep_sst_footer_build: null out");
  for (uint32_t j = 0; j < kvsep::sstw::kFooter; ++j)
    out[j] = char(kvsep::sstw::footer_byte(j, meta_off, meta_len, index_off, index_len));
  return KVSEP_OK;
}

uint64_t kvsep_log_accept(const uint64_t* off, const uint8_t* ok, uint64_t count, uint64_t n, uint8_t* accept) {
  uint64_t dropped = 0, dead_block = ~0ull;
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t hdr = off[i] - 6, blk = hdr / kLogBlock;
    if (blk == dead_block) {  // already dropped with the buffer
      accept[i] = 0;
      continue;
    }
    if (ok[i]) {
      accept[i] = 1;
      continue;
    }
    accept[i] = 0;
    const uint64_t end = (blk + 1) * kLogBlock < n ? (blk + 1) * kLogBlock : n;
    dropped += end - hdr;  // drop_size = buffer_.size() (:255-257)
    dead_block = blk;
  }
  return dropped;
}

uint64_t kvsep_log_accept_gaps(const char* buf, uint64_t n, const uint8_t* ok, uint64_t count, uint8_t* accept,
                               uint8_t* gap, uint64_t* bad_length_bytes) {
  uint64_t k = 0, dropped = 0, bad_length = 0, dead_block = ~0ull;
  bool pending = false;  // a kBadRecord without a physical record since the last record
  bool stopped = false;  // the reader returned kEof: nothing after it is read
  log_scan(
      buf, n,
      [&](uint64_t p, uint64_t, uint8_t t) {
        const uint64_t i = k++, blk = p / kLogBlock;
        if (i >= count) return;
        if (stopped || blk == dead_block) {  // never read, or already dropped with the buffer
          accept[i] = 0;
          if (gap) gap[i] = 0;
          return;
        }
        if (gap) gap[i] = pending ? 1 : 0;
        pending = false;
        if (!ok[i]) {
          accept[i] = 0;
          const uint64_t end = (blk + 1) * kLogBlock < n ? (blk + 1) * kLogBlock : n;
          dropped += end - p;  // drop_size = buffer_.size() (:255-257)
          dead_block = blk;
        } else if (t == kLogEofCode) {  // :270-271 returns the type byte itself: 5 reads as kEof
          accept[i] = 0;
          stopped = true;
        } else {
          accept[i] = t == kLogBadRecordCode ? 0 : 1;  // ... and 6 as a kBadRecord nobody reports
        }
      },
      [&](uint64_t p, uint64_t end, bool zero) {
        const uint64_t blk = p / kLogBlock;
        if (stopped || blk == dead_block) return;  // the reader never parsed this far
        pending = true;
        // reported only while eof_ is unset, i.e. when the block was read in full (:227-235)
        if (!zero && end - blk * kLogBlock == kLogBlock) bad_length += end - p;
      });
  if (bad_length_bytes) *bad_length_bytes = bad_length;
  return dropped;
}

uint64_t kvsep_log_chains(const uint8_t* type, const uint8_t* accept, const uint8_t* gap, uint64_t count,
                          uint64_t* first, uint8_t* whole, uint64_t* nwhole) {
  namespace chain = kvsep::chain;
  const auto gap_at = [&](uint64_t i) { return gap ? gap[i] : uint8_t(0); };
  uint64_t nchain = 0, nw = 0;
  bool in = false;  // a record is in progress (chain_run.h holds every rule)
  for (uint64_t i = 0; i < count; ++i) {
    const bool joins = chain::continues(type[i], accept[i], gap_at(i), in);
    if (!joins) first[nchain++] = i;
    in = chain::apply(in, chain::op_of(type[i], accept[i], gap_at(i)));
    const uint64_t nx = chain::next_index(i, count);
    if (chain::chain_ends(i, count, chain::continues(type[nx], accept[nx], gap_at(nx), in))) {
      whole[nchain - 1] = chain::whole_end(type[i], accept[i], joins) ? 1 : 0;
      nw += whole[nchain - 1];
    }
  }
  for (uint64_t k = nchain; k <= count; ++k) {
    if (chain::pads_first(k, nchain, count)) first[k] = chain::pad_first(count);
    if (chain::pads_whole(k, nchain, count)) whole[k] = 0;
  }
  if (nwhole) *nwhole = nw;
  return nchain;
}

}  // extern "C"
