// The checkpoint's header parser (libfm_amd/csrc/fmx_ckpt_format.h) against truncated and corrupted headers, on the CPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/ckpt_header_check.cpp -o ckpt_header_check
//     ./ckpt_header_check
//
// Headers are planned and encoded for every session kind, dense and sparse, with and without k1, num_factor 0 / 3 / 20; each must
// parse back to the same fields.  Then the parser is fed, from a heap buffer of EXACTLY the length it is told (so a read past the
// end is an AddressSanitizer report): every prefix of a header; every single-byte corruption of it (refused unless the byte is
// outside everything the header checksum covers -- there is no such byte); a file length off by one either way; and 20000 seeded
// random mutations with the header checksum RE-COMPUTED, so that the field checks behind the checksum are what refuses or accepts
// them -- whatever is accepted must re-plan to exactly its own section table and length.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../libfm_amd/csrc/fmx_ckpt_format.h"

namespace ck = fmx_ckpt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// parse from a heap copy of exactly `len` bytes
static bool parse_exact(const uint8_t* src, size_t len, uint64_t file_len, ck::Header* out, char* err, size_t err_len) {
  uint8_t* p = (uint8_t*)malloc(len ? len : 1);
  memcpy(p, src, len);
  const bool ok = ck::parse(len ? p : nullptr, len, file_len, out, err, err_len);
  free(p);
  return ok;
}

int main() {
  std::mt19937_64 rng(12345);
  char err[8];                                              // (shorter than any message: the parser must truncate, not overrun)
  char long_err[256];
  int headers = 0, accepted_mutations = 0;
  for (uint32_t session = 0; session <= 2; session++)
    for (uint32_t dense = 0; dense <= 1; dense++)
      for (uint32_t k1 = 0; k1 <= 1; k1++)
        for (uint32_t k : {0u, 3u, 20u}) {
          ck::Header h;
          h.session = session; h.num_attribute = 1001; h.num_factor = k; h.k0 = 1; h.k1 = k1;
          h.flags = dense ? ck::FLAG_DENSE : 0u;
          h.state_rows = session == 0 ? 0 : dense ? h.num_attribute : 37;
          for (uint32_t i = 0; i < ck::N_CONSTS; i++) h.consts[i] = session ? 0.25f * (float)(i + 1) : 0.f;
          const uint64_t total = ck::plan(&h);
          for (uint32_t i = 0; i < h.n_sections; i++) h.sec[i].checksum = rng();
          uint8_t buf[ck::HEADER_BYTES];
          ck::encode(h, buf);
          headers++;
          ck::Header back;
          CHECK(parse_exact(buf, sizeof(buf), total, &back, long_err, sizeof(long_err)), "a good header is refused: %s", long_err);
          CHECK(back.session == h.session && back.num_attribute == h.num_attribute && back.num_factor == h.num_factor && back.k1 == h.k1 &&
                back.flags == h.flags && back.state_rows == h.state_rows && back.n_sections == h.n_sections, "fields differ after a round trip");
          for (uint32_t i = 0; i < ck::MAX_SECTIONS; i++)
            CHECK(back.sec[i].kind == h.sec[i].kind && back.sec[i].offset == h.sec[i].offset && back.sec[i].bytes == h.sec[i].bytes &&
                  back.sec[i].checksum == h.sec[i].checksum, "section %u differs after a round trip", i);
          CHECK(memcmp(back.consts, h.consts, sizeof(h.consts)) == 0, "constants differ after a round trip");
          // truncation: every prefix, and a file one byte short / long
          for (size_t len = 0; len < sizeof(buf); len++)
            CHECK(!parse_exact(buf, len, total, &back, err, sizeof(err)), "a %zu-byte prefix is accepted", len);
          CHECK(!parse_exact(buf, sizeof(buf), total - 1, &back, err, sizeof(err)), "a file one byte short is accepted");
          CHECK(!parse_exact(buf, sizeof(buf), total + 1, &back, err, sizeof(err)), "a file one byte long is accepted");
          CHECK(parse_exact(buf, sizeof(buf), total, &back, nullptr, 0), "a NULL message buffer changes the verdict");
          // every single-byte corruption: the header checksum (or the magic / version check in front of it) refuses it
          for (size_t at = 0; at < sizeof(buf); at++) {
            uint8_t c[ck::HEADER_BYTES];
            memcpy(c, buf, sizeof(c));
            c[at] ^= (uint8_t)(1u << (rng() % 8));
            CHECK(!parse_exact(c, sizeof(c), total, &back, err, sizeof(err)), "a flipped bit in byte %zu is accepted", at);
          }
        }
  // random mutations behind a valid checksum
  for (int it = 0; it < 20000; it++) {
    ck::Header h;
    h.session = (uint32_t)(rng() % 3); h.num_attribute = 1 + rng() % 5000; h.num_factor = (uint32_t)(rng() % 40); h.k0 = 1; h.k1 = (uint32_t)(rng() % 2);
    h.flags = (rng() % 2) ? ck::FLAG_DENSE : 0u;
    h.state_rows = h.session == 0 ? 0 : (h.flags & ck::FLAG_DENSE) ? h.num_attribute : rng() % (h.num_attribute + 1);
    ck::plan(&h);
    uint8_t buf[ck::HEADER_BYTES];
    ck::encode(h, buf);
    const int n_mut = 1 + (int)(rng() % 3);
    for (int m = 0; m < n_mut; m++) {
      const size_t at = 8 + rng() % 272;                    // behind the magic, in front of the checksum
      switch (rng() % 3) {
        case 0: buf[at] = (uint8_t)rng(); break;
        case 1: buf[at] = 0xFF; break;
        default: buf[at] ^= (uint8_t)(1u << (rng() % 8));
      }
    }
    ck::put_u64(buf + 280, ck::checksum(buf, 280));
    const uint64_t file_len = (rng() % 4) ? ck::HEADER_BYTES + rng() % 1000000 : ~uint64_t(0) - rng() % 16;
    ck::Header got;
    uint64_t want_len = 0;
    bool ok = parse_exact(buf, sizeof(buf), file_len, &got, long_err, sizeof(long_err));
    if (!ok) {                                              // the same header with the length its own fields imply, if they are sane
      ck::Header probe;
      // try the planned length of the mutated fields: read them the way the parser does
      probe.session = ck::get_u32(buf + 12); probe.num_attribute = ck::get_u64(buf + 16); probe.num_factor = ck::get_u32(buf + 24);
      probe.k1 = ck::get_u32(buf + 32); probe.flags = ck::get_u32(buf + 36); probe.state_rows = ck::get_u64(buf + 72);
      if (probe.session <= 2 && probe.num_attribute && probe.num_attribute <= 0xFFFFFFFFull && probe.num_factor <= 1024 && probe.k1 <= 1 &&
          probe.state_rows <= probe.num_attribute) {
        want_len = ck::plan(&probe);
        ok = parse_exact(buf, sizeof(buf), want_len, &got, long_err, sizeof(long_err));
      }
    } else want_len = file_len;
    if (ok) {
      accepted_mutations++;
      ck::Header re = got;
      CHECK(ck::plan(&re) == want_len, "an accepted header does not re-plan to its length");
      CHECK(got.state_rows <= got.num_attribute && got.n_sections <= ck::MAX_SECTIONS, "an accepted header is out of range");
      for (uint32_t i = 0; i < ck::MAX_SECTIONS; i++)
        CHECK(re.sec[i].kind == got.sec[i].kind && re.sec[i].offset == got.sec[i].offset && re.sec[i].bytes == got.sec[i].bytes,
              "an accepted header's section %u is not the plan's", i);
      uint64_t end = ck::HEADER_BYTES;
      for (uint32_t i = 0; i < got.n_sections; i++) {
        CHECK(got.sec[i].offset == end, "section %u does not start where the one before ends", i);
        end = got.sec[i].offset + ck::padded(got.sec[i].bytes);
      }
      CHECK(end == want_len, "the sections do not add up to the file's length");
    }
  }
  // the checksum of a buffer whose length is no multiple of 8 reads nothing behind it
  for (size_t len = 0; len <= 40; len++) {
    uint8_t* p = (uint8_t*)malloc(len ? len : 1);
    for (size_t i = 0; i < len; i++) p[i] = (uint8_t)(i * 37 + 1);
    std::vector<uint8_t> padded(ck::padded(len), 0);
    if (len) memcpy(padded.data(), p, len);
    CHECK(ck::checksum(p, len) == ck::checksum(padded.data(), padded.size()), "the checksum of %zu bytes is not that of the padded bytes", len);
    free(p);
  }
  printf("%d headers, %d accepted mutations (the ones that changed only constants, checksums or agreed fields), %d failures\n",
         headers, accepted_mutations, failures);
  return failures ? 1 : 0;
}
