// The snapshot file's header parser (libfm_amd/csrc/fmx_snap_format.h) on the CPU, under the host compiler's sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/snap_header_check.cpp -o snap_header_check
//     ./snap_header_check              the self-test below
//     ./snap_header_check FILE         parse FILE's header as fmx_snapshot_info does: "ok <fields>" and exit 0, or "refused: <reason>"
//                                      and exit 2 (tests/test_snapshot_cpu.py feeds it files written by libfm_amd/compact.py and their
//                                      mutations)
//
// Self-test.  Headers are planned and encoded for both formats, dense and pruned, num_factor 0 / 5 / 40 / 100; each must parse back to
// the same fields.  Then the parser is fed, from a heap buffer of EXACTLY the length it is told (so a read past the end is an
// AddressSanitizer report): every prefix of a header; every single-bit corruption of it; a file length off by one either way; and
// 20000 seeded random mutations with the header checksum RE-COMPUTED, so that the field checks behind the checksum are what refuses
// or accepts them -- whatever is accepted must re-plan to exactly its own section table and length, with kept <= num_attribute and
// the block size of its num_factor.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../libfm_amd/csrc/fmx_snap_format.h"

namespace sn = fmx_snap;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// parse from a heap copy of exactly `len` bytes
static bool parse_exact(const uint8_t* src, size_t len, uint64_t file_len, sn::Header* out, char* err, size_t err_len) {
  uint8_t* p = (uint8_t*)malloc(len ? len : 1);
  memcpy(p, src, len);
  const bool ok = sn::parse(len ? p : nullptr, len, file_len, out, err, err_len);
  free(p);
  return ok;
}

static int parse_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("refused: cannot open %s\n", path); return 2; }
  fseek(f, 0, SEEK_END);
  const long file_len = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> buf(sn::HEADER_BYTES);
  const size_t got = fread(buf.data(), 1, buf.size(), f);
  fclose(f);
  sn::Header h;
  char err[256] = "";
  if (!parse_exact(buf.data(), got, (uint64_t)file_len, &h, err, sizeof(err))) { printf("refused: %s\n", err); return 2; }
  printf("ok format %u num_attribute %llu num_factor %u k0 %u k1 %u task %u pruned %u P %u kept %llu sections %u bytes %ld\n", h.format,
         (unsigned long long)h.num_attribute, h.num_factor, h.k0, h.k1, h.task, h.pruned, h.P, (unsigned long long)h.kept, h.n_sections, file_len);
  return 0;
}

static sn::Header make(uint32_t format, uint32_t pruned, uint32_t k, uint64_t n, uint64_t kept, uint64_t dead) {
  sn::Header h;
  h.format = format; h.num_attribute = n; h.num_factor = k; h.k0 = 1; h.k1 = 1; h.task = 1; h.min_target = -1.0; h.max_target = 1.0;
  h.pruned = pruned; h.P = format == sn::FORMAT_INT8 ? sn::int8_row_bytes(k) : 0u;
  h.kept = pruned ? kept : 0; h.nonfinite = 3; h.max_abs_err = 0.125; h.sum_sq_err = 2.5;
  h.dropped_dead = pruned ? dead : 0; h.dropped_unseen = pruned ? n - kept - dead : 0;
  return h;
}

int main(int argc, char** argv) {
  if (argc > 1) return parse_file(argv[1]);
  std::mt19937_64 rng(12345);
  char err[8];                                              // (shorter than any message: the parser must truncate, not overrun)
  char long_err[256];
  int headers = 0, accepted_mutations = 0;
  for (uint32_t format : {sn::FORMAT_BF16, sn::FORMAT_INT8})
    for (uint32_t pruned = 0; pruned <= 1; pruned++)
      for (uint32_t k : {0u, 5u, 40u, 100u}) {
        sn::Header h = make(format, pruned, k, 1001, 37, 900);
        const uint64_t total = sn::plan(&h);
        for (uint32_t i = 0; i < h.n_sections; i++) h.sec[i].checksum = rng();
        uint8_t buf[sn::HEADER_BYTES];
        sn::encode(h, buf);
        headers++;
        sn::Header back;
        CHECK(parse_exact(buf, sizeof(buf), total, &back, long_err, sizeof(long_err)), "a good header is refused: %s", long_err);
        CHECK(back.format == h.format && back.num_attribute == h.num_attribute && back.num_factor == h.num_factor && back.k0 == h.k0 &&
              back.k1 == h.k1 && back.task == h.task && back.pruned == h.pruned && back.P == h.P && back.kept == h.kept &&
              back.nonfinite == h.nonfinite && back.dropped_dead == h.dropped_dead && back.dropped_unseen == h.dropped_unseen &&
              back.n_sections == h.n_sections, "fields differ after a round trip");
        CHECK(back.min_target == h.min_target && back.max_target == h.max_target && back.max_abs_err == h.max_abs_err &&
              back.sum_sq_err == h.sum_sq_err, "doubles differ after a round trip");
        CHECK(h.n_sections == 2u + pruned + (format == sn::FORMAT_BF16 ? 1u : 0u), "%u sections", h.n_sections);
        for (uint32_t i = 0; i < sn::MAX_SECTIONS; i++)
          CHECK(back.sec[i].kind == h.sec[i].kind && back.sec[i].offset == h.sec[i].offset && back.sec[i].bytes == h.sec[i].bytes &&
                back.sec[i].checksum == h.sec[i].checksum, "section %u differs after a round trip", i);
        // truncation: every prefix, and a file one byte short / long
        for (size_t len = 0; len < sizeof(buf); len++)
          CHECK(!parse_exact(buf, len, total, &back, err, sizeof(err)), "a %zu-byte prefix is accepted", len);
        CHECK(!parse_exact(buf, sizeof(buf), total - 1, &back, err, sizeof(err)), "a file one byte short is accepted");
        CHECK(!parse_exact(buf, sizeof(buf), total + 1, &back, err, sizeof(err)), "a file one byte long is accepted");
        CHECK(parse_exact(buf, sizeof(buf), total, &back, nullptr, 0), "a NULL message buffer changes the verdict");
        // every single-bit corruption: the header checksum (or the magic / version check in front of it) refuses it
        for (size_t at = 0; at < sizeof(buf); at++) {
          uint8_t c[sn::HEADER_BYTES];
          memcpy(c, buf, sizeof(c));
          c[at] ^= (uint8_t)(1u << (rng() % 8));
          CHECK(!parse_exact(c, sizeof(c), total, &back, err, sizeof(err)), "a flipped bit in byte %zu is accepted", at);
        }
      }
  // random mutations behind a valid checksum
  for (int it = 0; it < 20000; it++) {
    const uint64_t n = 1 + rng() % 5000, kept = rng() % (n + 1), dead = rng() % (n - kept + 1);
    sn::Header h = make((rng() % 2) ? sn::FORMAT_BF16 : sn::FORMAT_INT8, (uint32_t)(rng() % 2), (uint32_t)(rng() % 140), n, kept, dead);
    sn::plan(&h);
    uint8_t buf[sn::HEADER_BYTES];
    sn::encode(h, buf);
    const int n_mut = 1 + (int)(rng() % 3);
    for (int m = 0; m < n_mut; m++) {
      const size_t at = 8 + rng() % (sn::SUM_AT - 8);       // behind the magic, in front of the checksum
      switch (rng() % 3) {
        case 0: buf[at] = (uint8_t)rng(); break;
        case 1: buf[at] = 0xFF; break;
        default: buf[at] ^= (uint8_t)(1u << (rng() % 8));
      }
    }
    sn::put_u64(buf + sn::SUM_AT, sn::checksum(buf, sn::SUM_AT));
    const uint64_t file_len = (rng() % 4) ? sn::HEADER_BYTES + rng() % 1000000 : ~uint64_t(0) - rng() % 16;
    sn::Header got;
    uint64_t want_len = 0;
    bool ok = parse_exact(buf, sizeof(buf), file_len, &got, long_err, sizeof(long_err));
    if (!ok) {                                              // the same header with the length its own fields imply, if they are sane
      sn::Header probe;
      probe.format = sn::get_u32(buf + 12); probe.num_attribute = sn::get_u64(buf + 16); probe.num_factor = sn::get_u32(buf + 24);
      probe.pruned = sn::get_u32(buf + 56); probe.P = sn::get_u32(buf + 60); probe.kept = sn::get_u64(buf + 64);
      if ((probe.format == sn::FORMAT_BF16 || probe.format == sn::FORMAT_INT8) && probe.num_attribute && probe.num_attribute <= 0xFFFFFFFFull &&
          probe.num_factor <= 1024 && probe.pruned <= 1 && probe.kept <= probe.num_attribute && probe.P <= 2048) {
        want_len = sn::plan(&probe);
        ok = parse_exact(buf, sizeof(buf), want_len, &got, long_err, sizeof(long_err));
      }
    } else want_len = file_len;
    if (ok) {
      accepted_mutations++;
      sn::Header re = got;
      CHECK(sn::plan(&re) == want_len, "an accepted header does not re-plan to its length");
      CHECK(got.kept <= got.num_attribute && (got.pruned || got.kept == 0) && got.n_sections <= sn::MAX_SECTIONS &&
            got.P == (got.format == sn::FORMAT_INT8 ? sn::int8_row_bytes(got.num_factor) : 0u) && got.k0 <= 1 && got.k1 <= 1 && got.task <= 1,
            "an accepted header is out of range");
      for (uint32_t i = 0; i < sn::MAX_SECTIONS; i++)
        CHECK(re.sec[i].kind == got.sec[i].kind && re.sec[i].offset == got.sec[i].offset && re.sec[i].bytes == got.sec[i].bytes,
              "an accepted header's section %u is not the plan's", i);
      uint64_t end = sn::HEADER_BYTES;
      for (uint32_t i = 0; i < got.n_sections; i++) {
        CHECK(got.sec[i].offset == end, "section %u does not start where the one before ends", i);
        end = got.sec[i].offset + sn::padded(got.sec[i].bytes);
      }
      CHECK(end == want_len, "the sections do not add up to the file's length");
    }
  }
  printf("%d headers, %d accepted mutations (the ones that changed only figures, checksums or agreed fields), %d failures\n",
         headers, accepted_mutations, failures);
  return failures ? 1 : 0;
}
