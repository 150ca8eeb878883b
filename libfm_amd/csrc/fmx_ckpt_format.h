// fmx_ckpt_format.h -- the byte layout of a binary checkpoint (include/fmx.h "fmx_checkpoint_*"): the header's
// fields, the plan of the sections that follow it, and the parser that refuses everything a load must refuse before the first byte
// reaches the device.  HOST ONLY: nothing from HIP is included, so fmx_checkpoint_info needs no device and
// scripts/ckpt_header_check.cpp builds with the host compiler and its sanitizers.  libfm_amd/checkpoint.py restates the same layout.
//
// Little-endian throughout.  The header is HEADER_BYTES = 288 bytes:
//     0  char[8]  magic "FMXCKPT\0"
//     8  u32      version (1)                  12  u32  session: 0 none, 1 AdaGrad, 2 FTRL
//    16  u64      num_attribute                24  u32  num_factor     28  u32  k0     32  u32  k1
//    36  u32      flags the file was saved with (FMX_CKPT_DENSE_STATE | FMX_CKPT_MODEL_ONLY)
//    40  f32[8]   the session's constants as the kernels took them (zeros without a session)
//                   AdaGrad: eta, init_acc          FTRL: 1 / alpha, beta, l1_w, l1_v, l2_w, l2_v, init_acc
//    72  u64      state_rows                   80  u32  number of sections     84  u32  0
//    88  6 x {u32 kind, u32 0, u64 offset, u64 bytes, u64 checksum}   (unused entries are all zero)
//   280  u64      checksum of bytes 0 .. 279
// The sections follow in the order of their kinds, the first at 288, each padded with zero bytes to a multiple of 8:
//     1 w0   one f64                                    2 w   num_attribute f32, only with k1
//     3 V    num_attribute rows of num_factor f32        4 ids state_rows u32, strictly ascending; absent when dense or without a session
//     5 z    FTRL only / 6 n: state_rows rows of 1 + num_factor f32, the linear coordinate's value first
// `bytes` is the length without the padding; the checksum runs over the padded words (checksum() below).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace fmx_ckpt {

constexpr uint32_t VERSION = 1, HEADER_BYTES = 288, MAX_SECTIONS = 6, N_CONSTS = 8;
constexpr uint32_t FLAG_DENSE = 1u, FLAG_MODEL_ONLY = 2u, KNOWN_FLAGS = 3u;
constexpr uint32_t SESSION_NONE = 0, SESSION_ADAGRAD = 1, SESSION_FTRL = 2;
enum : uint32_t { SEC_W0 = 1, SEC_W = 2, SEC_V = 3, SEC_IDS = 4, SEC_Z = 5, SEC_N = 6 };
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ULL;
static const char MAGIC[8] = {'F', 'M', 'X', 'C', 'K', 'P', 'T', '\0'};

struct Section { uint32_t kind = 0; uint64_t offset = 0, bytes = 0, checksum = 0; };
struct Header {
  uint32_t version = VERSION, session = 0;
  uint64_t num_attribute = 0;
  uint32_t num_factor = 0, k0 = 0, k1 = 0, flags = 0;
  float    consts[N_CONSTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t state_rows = 0;
  uint32_t n_sections = 0;
  Section  sec[MAX_SECTIONS];
};

inline const char* section_name(uint32_t kind) {
  static const char* const names[] = {"?", "w0", "w", "V", "state ids", "state z", "state n"};
  return kind <= SEC_N ? names[kind] : "?";
}

// the mix64 of fmx_kernels.h, restated so that this header stays free of HIP (tests/test_gpu_checkpoint.py holds the device's sums,
// this one and checkpoint.py's together: one file, three readers)
inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27; x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  return x;
}
inline uint64_t word_term(uint64_t u, uint64_t i) { return mix64(u ^ (i * GOLDEN)); }

inline uint64_t get_u64(const uint8_t* p) { uint64_t v = 0; for (int i = 7; i >= 0; i--) v = (v << 8) | p[i]; return v; }
inline uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void put_u64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) { p[i] = (uint8_t)(v & 0xFF); v >>= 8; } }
inline void put_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) { p[i] = (uint8_t)(v & 0xFF); v >>= 8; } }

// the sum mod 2^64 of word_term over the 8-byte words of `bytes` bytes padded with zeros to a multiple of 8; word indices start at first_word
inline uint64_t checksum(const uint8_t* p, uint64_t bytes, uint64_t first_word = 0) {
  uint64_t s = 0, i = 0;
  for (; (i + 1) * 8 <= bytes; i++) s += word_term(get_u64(p + i * 8), first_word + i);
  if (i * 8 < bytes) {
    uint8_t last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    memcpy(last, p + i * 8, (size_t)(bytes - i * 8));
    s += word_term(get_u64(last), first_word + i);
  }
  return s;
}

inline uint64_t padded(uint64_t bytes) { return (bytes + 7u) & ~uint64_t(7); }

// kinds, offsets and lengths of the sections that the header's geometry, session, flags and state_rows imply (checksums zeroed);
// returns the file's length.  The geometry has been bounded by the caller (parse) or comes from a handle, so nothing overflows:
// num_attribute < 2^32, num_factor <= 1024.
inline uint64_t plan(Header* h) {
  const bool dense = (h->flags & FLAG_DENSE) != 0;
  const uint64_t n = h->num_attribute, row = (uint64_t)(1 + h->num_factor) * 4;
  uint32_t ns = 0;
  uint64_t off = HEADER_BYTES;
  auto add = [&](uint32_t kind, uint64_t bytes) {
    h->sec[ns].kind = kind; h->sec[ns].offset = off; h->sec[ns].bytes = bytes; h->sec[ns].checksum = 0;
    off += padded(bytes); ns++;
  };
  add(SEC_W0, 8);
  if (h->k1) add(SEC_W, n * 4);
  add(SEC_V, n * (uint64_t)h->num_factor * 4);
  if (h->session != SESSION_NONE) {
    if (!dense) add(SEC_IDS, h->state_rows * 4);
    if (h->session == SESSION_FTRL) add(SEC_Z, h->state_rows * row);
    add(SEC_N, h->state_rows * row);
  }
  h->n_sections = ns;
  for (uint32_t i = ns; i < MAX_SECTIONS; i++) h->sec[i] = Section();
  return off;
}

inline void encode(const Header& h, uint8_t out[HEADER_BYTES]) {
  memset(out, 0, HEADER_BYTES);
  memcpy(out, MAGIC, 8);
  put_u32(out + 8, h.version); put_u32(out + 12, h.session);
  put_u64(out + 16, h.num_attribute);
  put_u32(out + 24, h.num_factor); put_u32(out + 28, h.k0); put_u32(out + 32, h.k1); put_u32(out + 36, h.flags);
  for (uint32_t i = 0; i < N_CONSTS; i++) { uint32_t b; memcpy(&b, &h.consts[i], 4); put_u32(out + 40 + 4 * i, b); }
  put_u64(out + 72, h.state_rows);
  put_u32(out + 80, h.n_sections);
  for (uint32_t i = 0; i < MAX_SECTIONS; i++) {
    uint8_t* s = out + 88 + 32 * i;
    put_u32(s, h.sec[i].kind); put_u64(s + 8, h.sec[i].offset); put_u64(s + 16, h.sec[i].bytes); put_u64(s + 24, h.sec[i].checksum);
  }
  put_u64(out + 280, checksum(out, 280));
}

// parse and validate the first `len` bytes of a file that is file_len bytes long.  false + a message in err for: fewer than
// HEADER_BYTES bytes, bad magic, a version other than 1, a header checksum mismatch, unknown flags or session, a geometry outside
// what a handle can have, state_rows > num_attribute (or != num_attribute when dense, != 0 without a session), a section table that
// is not the plan of those fields, a planned length other than file_len.  Reads nothing beyond buf[len - 1].
inline bool parse(const uint8_t* buf, size_t len, uint64_t file_len, Header* out, char* err, size_t err_len) {
  auto bad = [&](const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    if (err && err_len) snprintf(err, err_len, fmt, a, b);
    return false;
  };
  if (!buf || len < HEADER_BYTES) return bad("the file is shorter than a checkpoint header (%llu of %llu bytes)", (unsigned long long)len, HEADER_BYTES);
  if (memcmp(buf, MAGIC, 8) != 0) return bad("bad magic: not a checkpoint file");
  Header h;
  h.version = get_u32(buf + 8);
  if (h.version != VERSION) return bad("checkpoint version %llu, this library reads version %llu", h.version, VERSION);
  if (get_u64(buf + 280) != checksum(buf, 280)) return bad("the header's checksum does not match");
  h.session = get_u32(buf + 12);
  h.num_attribute = get_u64(buf + 16);
  h.num_factor = get_u32(buf + 24); h.k0 = get_u32(buf + 28); h.k1 = get_u32(buf + 32); h.flags = get_u32(buf + 36);
  for (uint32_t i = 0; i < N_CONSTS; i++) { const uint32_t b = get_u32(buf + 40 + 4 * i); memcpy(&h.consts[i], &b, 4); }
  h.state_rows = get_u64(buf + 72);
  h.n_sections = get_u32(buf + 80);
  if (h.session > SESSION_FTRL) return bad("unknown session kind %llu", h.session);
  if (h.flags & ~KNOWN_FLAGS) return bad("unknown flags 0x%llx", h.flags);
  if (h.num_attribute == 0 || h.num_attribute > 0xFFFFFFFFull) return bad("num_attribute %llu is outside 1 .. 2^32 - 1", h.num_attribute);
  if (h.num_factor > 1024) return bad("num_factor %llu is above 1024", h.num_factor);
  if (h.k0 > 1 || h.k1 > 1) return bad("k0 / k1 are %llu / %llu, not 0 or 1", h.k0, h.k1);
  if (h.state_rows > h.num_attribute) return bad("state_rows %llu > num_attribute %llu", h.state_rows, h.num_attribute);
  if (h.session == SESSION_NONE && h.state_rows != 0) return bad("state_rows %llu without a session", h.state_rows);
  if (h.session != SESSION_NONE && (h.flags & FLAG_DENSE) && h.state_rows != h.num_attribute)
    return bad("a dense file with state_rows %llu != num_attribute %llu", h.state_rows, h.num_attribute);
  if (h.n_sections > MAX_SECTIONS) return bad("%llu sections, at most %llu", h.n_sections, MAX_SECTIONS);
  Header want = h;
  const uint64_t total = plan(&want);
  if (want.n_sections != h.n_sections) return bad("the section table has %llu entries, the header's fields imply %llu", h.n_sections, want.n_sections);
  for (uint32_t i = 0; i < MAX_SECTIONS; i++) {
    const uint8_t* s = buf + 88 + 32 * i;
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

}  // namespace fmx_ckpt
