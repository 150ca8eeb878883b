// fmx_snap_format.h -- the byte layout of a serving snapshot file (include/fmx.h "fmx_compact_save"): the
// header's fields, the plan of the sections that follow it, and the parser that refuses everything a load must refuse before the
// first byte reaches the device.  HOST ONLY, like fmx_ckpt_format.h, whose conventions, checksum and byte helpers it uses: nothing
// from HIP is included, so fmx_snapshot_info needs no device and scripts/snap_header_check.cpp builds with the host compiler and its
// sanitizers.  libfm_amd/compact.py (write_snapshot / read_snapshot) restates the same layout.
//
// Little-endian throughout.  The header is HEADER_BYTES = 256 bytes:
//     0  char[8]  magic "FMXSNAP\0"
//     8  u32      version (1)                  12  u32  format: FMX_COMPACT_BF16 (1) or FMX_COMPACT_INT8 (3)
//    16  u64      num_attribute                24  u32  num_factor     28  u32  k0     32  u32  k1     36  u32  task (0 / 1)
//    40  f64      min_target                   48  f64  max_target
//    56  u32      pruned (0 / 1)               60  u32  P: bytes of an int8 block, compact8_row_bytes(num_factor); 0 for bf16
//    64  u64      kept: rows of a pruned snapshot, 0 otherwise
//    72  u64      nonfinite    80  f64  max_abs_err    88  f64  sum_sq_err     (fmx_compact_info, as the snapshot was taken)
//    96  u64      dropped_dead                104  u64  dropped_unseen         (fmx_compact_prune_info; its other two counts are
//                                                                               num_attribute and kept.  Zeros when not pruned)
//   112  u32      number of sections          116  u32  0
//   120  4 x {u32 kind, u32 0, u64 offset, u64 bytes, u64 checksum}   (unused entries are all zero)
//   248  u64      checksum of bytes 0 .. 247
// The sections follow in the order of their kinds, the first at 256, each padded with zero bytes to a multiple of 8.  With
// rows = kept for a pruned snapshot and num_attribute otherwise:
//     1 w0    one f64
//     2 dir   pruned only: ceil(num_attribute / 32) pairs {u32 bits, u32 base}, as the device holds them
//     3 rows  int8 only: rows blocks of P bytes, verbatim (scale, w, codes, zeros up to P)
//     4 w     bf16 only: rows f32
//     5 V     bf16 only: rows rows of num_factor u16 -- the row padding of the device table is NOT in the file
// `bytes` is the length without the padding; the checksum runs over the padded words (fmx_ckpt::checksum).
#pragma once
#include "fmx_ckpt_format.h"

namespace fmx_snap {

using fmx_ckpt::Section;
using fmx_ckpt::checksum;
using fmx_ckpt::get_u32;
using fmx_ckpt::get_u64;
using fmx_ckpt::put_u32;
using fmx_ckpt::put_u64;
using fmx_ckpt::padded;

constexpr uint32_t VERSION = 1, HEADER_BYTES = 256, MAX_SECTIONS = 4, TABLE_AT = 120, SUM_AT = 248;
constexpr uint32_t FORMAT_BF16 = 1, FORMAT_INT8 = 3;      // FMX_COMPACT_*
enum : uint32_t { SEC_W0 = 1, SEC_DIR = 2, SEC_ROWS = 3, SEC_W = 4, SEC_V = 5 };
static const char MAGIC[8] = {'F', 'M', 'X', 'S', 'N', 'A', 'P', '\0'};

struct Header {
  uint32_t version = VERSION, format = 0;
  uint64_t num_attribute = 0;
  uint32_t num_factor = 0, k0 = 0, k1 = 0, task = 0;
  double   min_target = 0.0, max_target = 0.0;
  uint32_t pruned = 0, P = 0;
  uint64_t kept = 0, nonfinite = 0;
  double   max_abs_err = 0.0, sum_sq_err = 0.0;
  uint64_t dropped_dead = 0, dropped_unseen = 0;
  uint32_t n_sections = 0;
  Section  sec[MAX_SECTIONS];
};

inline const char* section_name(uint32_t kind) {
  static const char* const names[] = {"?", "w0", "dir", "rows", "w", "V"};
  return kind <= SEC_V ? names[kind] : "?";
}

// fmx_compact_kernels.h compact8_row_bytes, restated so that this header stays free of HIP (scripts/snap_header_check.cpp and
// tests/test_snapshot_cpu.py hold it against compact.row_bytes)
inline uint32_t int8_row_bytes(uint32_t k) {
  uint32_t need = k + 8u, p = 8u;
  if (need > 128u) return (need + 63u) / 64u * 64u;
  while (p < need) p <<= 1;
  return p;
}

inline uint64_t rows_of(const Header& h) { return h.pruned ? h.kept : h.num_attribute; }

// kinds, offsets and lengths of the sections that the header's fields imply (checksums zeroed); returns the file's length.  The
// geometry has been bounded by the caller (parse) or comes from a handle, so nothing overflows: num_attribute < 2^32, num_factor <= 1024.
inline uint64_t plan(Header* h) {
  const uint64_t rows = rows_of(*h);
  uint32_t ns = 0;
  uint64_t off = HEADER_BYTES;
  auto add = [&](uint32_t kind, uint64_t bytes) {
    h->sec[ns].kind = kind; h->sec[ns].offset = off; h->sec[ns].bytes = bytes; h->sec[ns].checksum = 0;
    off += padded(bytes); ns++;
  };
  add(SEC_W0, 8);
  if (h->pruned) add(SEC_DIR, (h->num_attribute + 31) / 32 * 8);
  if (h->format == FORMAT_INT8) add(SEC_ROWS, rows * (uint64_t)h->P);
  else { add(SEC_W, rows * 4); add(SEC_V, rows * (uint64_t)h->num_factor * 2); }
  h->n_sections = ns;
  for (uint32_t i = ns; i < MAX_SECTIONS; i++) h->sec[i] = Section();
  return off;
}

inline void put_f64(uint8_t* p, double v) { uint64_t u; memcpy(&u, &v, 8); put_u64(p, u); }
inline double get_f64(const uint8_t* p) { const uint64_t u = get_u64(p); double v; memcpy(&v, &u, 8); return v; }

inline void encode(const Header& h, uint8_t out[HEADER_BYTES]) {
  memset(out, 0, HEADER_BYTES);
  memcpy(out, MAGIC, 8);
  put_u32(out + 8, h.version); put_u32(out + 12, h.format);
  put_u64(out + 16, h.num_attribute);
  put_u32(out + 24, h.num_factor); put_u32(out + 28, h.k0); put_u32(out + 32, h.k1); put_u32(out + 36, h.task);
  put_f64(out + 40, h.min_target); put_f64(out + 48, h.max_target);
  put_u32(out + 56, h.pruned); put_u32(out + 60, h.P);
  put_u64(out + 64, h.kept); put_u64(out + 72, h.nonfinite);
  put_f64(out + 80, h.max_abs_err); put_f64(out + 88, h.sum_sq_err);
  put_u64(out + 96, h.dropped_dead); put_u64(out + 104, h.dropped_unseen);
  put_u32(out + 112, h.n_sections);
  for (uint32_t i = 0; i < MAX_SECTIONS; i++) {
    uint8_t* s = out + TABLE_AT + 32 * i;
    put_u32(s, h.sec[i].kind); put_u64(s + 8, h.sec[i].offset); put_u64(s + 16, h.sec[i].bytes); put_u64(s + 24, h.sec[i].checksum);
  }
  put_u64(out + SUM_AT, checksum(out, SUM_AT));
}

// parse and validate the first `len` bytes of a file that is file_len bytes long.  false + a message in err (it names the field) for:
// fewer than HEADER_BYTES bytes, bad magic, a version other than 1, a header checksum mismatch, an unknown format, a geometry or task
// outside what a handle can have, pruned not 0 / 1, kept > num_attribute, kept without pruned, P other than the format's, counts of a
// pruned snapshot that do not add up to num_attribute (or counts without pruned), a section table that is not the plan of those
// fields, a planned length other than file_len.  Reads nothing beyond buf[len - 1].
inline bool parse(const uint8_t* buf, size_t len, uint64_t file_len, Header* out, char* err, size_t err_len) {
  auto bad = [&](const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    if (err && err_len) snprintf(err, err_len, fmt, a, b);
    return false;
  };
  if (!buf || len < HEADER_BYTES) return bad("the file is shorter than a snapshot header (%llu of %llu bytes)", (unsigned long long)len, HEADER_BYTES);
  if (memcmp(buf, MAGIC, 8) != 0) return bad("bad magic: not a snapshot file");
  Header h;
  h.version = get_u32(buf + 8);
  if (h.version != VERSION) return bad("snapshot version %llu, this library reads version %llu", h.version, VERSION);
  if (get_u64(buf + SUM_AT) != checksum(buf, SUM_AT)) return bad("the header's checksum does not match");
  h.format = get_u32(buf + 12);
  h.num_attribute = get_u64(buf + 16);
  h.num_factor = get_u32(buf + 24); h.k0 = get_u32(buf + 28); h.k1 = get_u32(buf + 32); h.task = get_u32(buf + 36);
  h.min_target = get_f64(buf + 40); h.max_target = get_f64(buf + 48);
  h.pruned = get_u32(buf + 56); h.P = get_u32(buf + 60);
  h.kept = get_u64(buf + 64); h.nonfinite = get_u64(buf + 72);
  h.max_abs_err = get_f64(buf + 80); h.sum_sq_err = get_f64(buf + 88);
  h.dropped_dead = get_u64(buf + 96); h.dropped_unseen = get_u64(buf + 104);
  h.n_sections = get_u32(buf + 112);
  if (h.format != FORMAT_BF16 && h.format != FORMAT_INT8) return bad("unknown format %llu (1 bf16, 3 int8)", h.format);
  if (h.num_attribute == 0 || h.num_attribute > 0xFFFFFFFFull) return bad("num_attribute %llu is outside 1 .. 2^32 - 1", h.num_attribute);
  if (h.num_factor > 1024) return bad("num_factor %llu is above 1024", h.num_factor);
  if (h.k0 > 1 || h.k1 > 1) return bad("k0 / k1 are %llu / %llu, not 0 or 1", h.k0, h.k1);
  if (h.task > 1) return bad("task %llu is neither regression (0) nor classification (1)", h.task);
  if (h.pruned > 1) return bad("pruned is %llu, not 0 or 1", h.pruned);
  if (h.kept > h.num_attribute) return bad("kept %llu > num_attribute %llu", h.kept, h.num_attribute);
  if (!h.pruned && h.kept != 0) return bad("kept %llu without pruned", h.kept);
  const uint32_t want_P = h.format == FORMAT_INT8 ? int8_row_bytes(h.num_factor) : 0u;
  if (h.P != want_P) return bad("P (bytes of an int8 block) is %llu, the format and num_factor imply %llu", h.P, want_P);
  if (!h.pruned && (h.dropped_dead != 0 || h.dropped_unseen != 0)) return bad("dropped_dead / dropped_unseen %llu / %llu without pruned", h.dropped_dead, h.dropped_unseen);
  if (h.pruned && (h.dropped_dead > h.num_attribute || h.dropped_unseen > h.num_attribute ||
                   h.kept + h.dropped_dead + h.dropped_unseen != h.num_attribute))
    return bad("kept + dropped_dead + dropped_unseen is not num_attribute (dropped_dead %llu, dropped_unseen %llu)", h.dropped_dead, h.dropped_unseen);
  if (get_u32(buf + 116) != 0) return bad("the reserved word at byte 116 is %llu, not 0", get_u32(buf + 116));
  if (h.n_sections > MAX_SECTIONS) return bad("%llu sections, at most %llu", h.n_sections, MAX_SECTIONS);
  Header want = h;
  const uint64_t total = plan(&want);
  if (want.n_sections != h.n_sections) return bad("the section table has %llu entries, the header's fields imply %llu", h.n_sections, want.n_sections);
  for (uint32_t i = 0; i < MAX_SECTIONS; i++) {
    const uint8_t* s = buf + TABLE_AT + 32 * i;
    h.sec[i].kind = get_u32(s); h.sec[i].offset = get_u64(s + 8); h.sec[i].bytes = get_u64(s + 16); h.sec[i].checksum = get_u64(s + 24);
    if (h.sec[i].kind != want.sec[i].kind || h.sec[i].offset != want.sec[i].offset || h.sec[i].bytes != want.sec[i].bytes ||
        get_u32(s + 4) != 0 || (i >= h.n_sections && h.sec[i].checksum != 0)) {
      if (err && err_len) snprintf(err, err_len, "section table entry %u (%s) does not match the header's fields", i, section_name(want.sec[i].kind));
      return false;
    }
  }
  if (total != file_len) return bad("the sections end at byte %llu but the file has %llu bytes (truncated?)", total, file_len);
  *out = h;
  return true;
}

}  // namespace fmx_snap
