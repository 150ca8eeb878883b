// The host side of device memory and table placement (libfm_amd/csrc/fmx_place_plan.h) against its specification, on the CPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/place_plan_check.cpp -o place_plan_check
//     ./place_plan_check
//
// 1. mapping order: every T <= 24 and every stock of X, Y, other and straddling chunks up to T + 2 each, against a restatement of
//    the rule by positions, plus its properties;  2. the prefix rule of the arena cache against a scan;  3. layout and pool bound
//    on random sizes;  4. build_arena against a fake device whose physical chunks come in runs of one class, with straddling chunks
//    at run borders and +-2 % noise on the probe times;  5. the same cases with the n-th call of the virtual-memory API failing,
//    for every n, and the chunk-by-chunk range of a big allocation with every call failing in turn: either the result is complete
//    or nothing is outstanding on the device.  Exits non-zero at the first disagreement; the last line counts the cases.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "../libfm_amd/csrc/fmx_place_plan.h"

using namespace fmx;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
                                             fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
static const size_t CH = ARENA_CHUNK;
static const uint64_t RS[5] = {16, 32, 64, 128, 256}, KPS[7] = {1, 2, 8, 32, 64, 128, 256};
static const size_t RUNS[5] = {1, 2, 5, 16, 64};

// ---- the fake device -------------------------------------------------------------------------------------------------------------
// Physical chunk number p (in order of creation) has class cls_of[p], or -1 where it straddles a border.  Addresses are numbers that
// nothing dereferences.  Every call counts; call number fail_at (1-based) fails without effect -- a failing unmap, release or
// free_address LOSES what it was given, which is then no longer counted as outstanding.
struct FakeDevice : Vm, Probe {
  enum Kind { RESERVE, FREE_ADDRESS, CREATE, RELEASE, MAP, UNMAP, SET_ACCESS };
  struct Mapping { size_t bytes; void* hnd; bool lost; };
  struct Handle { size_t bytes; int phys; };
  std::vector<int> cls_of;
  size_t capacity = SIZE_MAX;                               // live handles the device has memory for
  size_t calls = 0, fail_at = 0;
  int failed_kind = -1; size_t failed_handles = 0; bool failed_in_first = false;   // what failed, with how many handles created so far
  std::map<uintptr_t, size_t> reservations;                 // base -> bytes
  std::map<uintptr_t, Mapping> mappings;                    // address -> what is mapped there
  std::map<void*, Handle> handles;
  std::vector<uintptr_t> reserve_order;
  uintptr_t next_va = (uintptr_t)1 << 40;
  size_t created = 0;
  std::mt19937_64 noise{1};
  std::vector<uint32_t> pair_probes, alone_probes;          // per physical chunk: probes it was the SECOND argument of

  bool fails(Kind k, bool in_first = false) {
    if (++calls != fail_at) return false;
    failed_kind = k; failed_handles = created; failed_in_first = in_first;
    return true;
  }
  bool in_first_range(void* at) const { return !reserve_order.empty() && (uintptr_t)at >= reserve_order[0] && (uintptr_t)at < reserve_order[0] + reservations.at(reserve_order[0]); }
  int reserve(void** va, size_t bytes, size_t align) override {
    if (fails(RESERVE)) return 2;
    next_va = (next_va + align - 1) / align * align;
    *va = (void*)next_va; reservations[next_va] = bytes; reserve_order.push_back(next_va); next_va += bytes + CH;
    return 0;
  }
  int free_address(void* va, size_t bytes) override {
    auto it = reservations.find((uintptr_t)va);
    CHECK(it != reservations.end() && it->second == bytes, "free_address of something never reserved, or with another size");
    for (auto m = mappings.begin(); m != mappings.end();) {
      const bool outside = m->first + m->second.bytes <= (uintptr_t)va || m->first >= (uintptr_t)va + bytes;
      CHECK(outside || m->second.lost, "free_address under a live mapping");
      m = outside ? std::next(m) : mappings.erase(m);
    }
    reservations.erase(it);
    return fails(FREE_ADDRESS) ? 2 : 0;
  }
  int create(void** hnd, size_t bytes) override {
    if (fails(CREATE) || handles.size() >= capacity) return 2;
    CHECK(created < cls_of.size(), "the fake device ran out of described memory");
    *hnd = (void*)(uintptr_t)(0x1000 + created);
    handles[*hnd] = Handle{bytes, (int)created++};
    pair_probes.push_back(0); alone_probes.push_back(0);
    return 0;
  }
  int release(void* hnd) override {
    CHECK(handles.erase(hnd) == 1, "release of a handle that is not live (released twice?)");
    return fails(RELEASE) ? 2 : 0;
  }
  int map(void* at, size_t bytes, void* hnd) override {
    if (fails(MAP, in_first_range(at))) return 2;
    CHECK(handles.count(hnd) && handles[hnd].bytes == bytes, "map of a handle that is not live, or with another size");
    bool inside = false;
    for (auto& r : reservations) inside |= (uintptr_t)at >= r.first && (uintptr_t)at + bytes <= r.first + r.second;
    CHECK(inside, "map outside every reservation");
    for (auto& m : mappings) {
      CHECK(m.first + m.second.bytes <= (uintptr_t)at || m.first >= (uintptr_t)at + bytes, "map over a live mapping");
      CHECK(m.second.hnd != hnd, "a handle mapped twice at the same time");
    }
    mappings[(uintptr_t)at] = Mapping{bytes, hnd, false};
    return 0;
  }
  int unmap(void* at, size_t bytes) override {
    auto it = mappings.find((uintptr_t)at);
    CHECK(it != mappings.end() && it->second.bytes == bytes, "unmap of something that is not mapped (unmapped twice?)");
    if (fails(UNMAP)) { it->second.lost = true; return 2; }       // (stays until it is unmapped again or its range is freed)
    mappings.erase(it);
    return 0;
  }
  int set_access(void* at, size_t bytes) override {
    if (fails(SET_ACCESS, in_first_range(at) && bytes == CH)) return 2;
    CHECK(mapped_within(at, bytes) == bytes, "set_access over a range that is not wholly mapped");
    return 0;
  }
  int phys_at(void* at) {
    auto it = mappings.find((uintptr_t)at);
    CHECK(it != mappings.end(), "a probe of an address nothing is mapped at");
    const auto h = handles.find(it->second.hnd);
    return h != handles.end() ? h->second.phys : (int)((uintptr_t)it->second.hnd - 0x1000);   // (a handle given up lives on through its mapping)
  }
  size_t mapped_within(void* at, size_t bytes) const {
    size_t covered = 0;
    for (auto& m : mappings) if (m.first >= (uintptr_t)at && m.first + m.second.bytes <= (uintptr_t)at + bytes) covered += m.second.bytes;
    return covered;
  }
  int zero(void* at, size_t bytes) override { CHECK(mapped_within(at, bytes) == bytes, "a write to a range that is not wholly mapped"); return 0; }
  int sync() override { return 0; }
  // one chunk alone, or two of one class: 1 ms; two classes together, or anything with a straddling chunk: 0.8 ms; +-2 %
  int pair_ms(void* a, void* b, float* ms) override {
    const int pa = phys_at(a), pb = phys_at(b);
    float t;
    if (pa == pb) { alone_probes[pb]++; t = cls_of[pa] < 0 ? 0.8f : 1.0f; }
    else { pair_probes[pb]++; t = (cls_of[pa] >= 0 && cls_of[pa] == cls_of[pb]) ? 1.0f : 0.8f; }
    *ms = t * (0.98f + 0.04f * (float)(noise() % 1001) / 1000.f);
    return 0;
  }
  bool nothing_outstanding() const { return reservations.empty() && mappings.empty() && handles.empty(); }
};

// ---- 1. the mapping order, restated by positions --------------------------------------------------------------------------------
static bool order_by_positions(size_t nX, size_t nY, size_t nO, size_t nS, size_t T, std::vector<size_t>* out, std::vector<uint8_t>* cls) {
  out->clear(); cls->clear();
  const size_t ny = std::min(nY, T / 2), nx = std::min(nX, T - ny);
  size_t tx = 0, ty = 0, to = 0, ts = 0;
  for (size_t c = 0; c < T; c++) {
    const bool y_turn = ((c + 1) * ny) / T > (c * ny) / T && ty < ny;
    if (y_turn) { out->push_back(1000 + ty++); cls->push_back(1); }
    else if (tx < nx) { out->push_back(tx++); cls->push_back(0); }
    else if (ty < nY) { out->push_back(1000 + ty++); cls->push_back(1); }
    else if (to < nO) { out->push_back(2000 + to++); cls->push_back(2); }
    else if (ts < nS) { out->push_back(3000 + ts++); cls->push_back(2); }
    else return false;
  }
  return true;
}
static size_t check_mapping_order() {
  size_t n = 0;
  std::vector<size_t> X, Y, rest, pick, want;
  std::vector<uint8_t> cls, want_cls;
  for (size_t T = 1; T <= 24; T++)
    for (size_t nX = 0; nX <= T + 2; nX++) for (size_t nY = 0; nY <= T + 2; nY++)
      for (size_t nO = 0; nO <= T + 2; nO++) for (size_t nS = 0; nS <= T + 2; nS++, n++) {
        X.clear(); Y.clear(); rest.clear();
        for (size_t i = 0; i < nX; i++) X.push_back(i);
        for (size_t i = 0; i < nY; i++) Y.push_back(1000 + i);
        for (size_t i = 0; i < nO; i++) rest.push_back(2000 + i);
        for (size_t i = 0; i < nS; i++) rest.push_back(3000 + i);
        uint32_t per[2] = {77, 77};
        const bool ok = mapping_order(X, Y, rest, T, &pick, &cls, per);
        const bool want_ok = order_by_positions(nX, nY, nO, nS, T, &want, &want_cls);
        CHECK(ok == want_ok && ok == (nX + nY + nO + nS >= T), "T %zu stock %zu %zu %zu %zu: success %d, by positions %d", T, nX, nY, nO, nS, ok, want_ok);
        if (!ok) continue;
        CHECK(pick == want && cls == want_cls, "T %zu stock %zu %zu %zu %zu: another order than by positions", T, nX, nY, nO, nS);
        std::vector<size_t> s(pick); std::sort(s.begin(), s.end());
        CHECK(pick.size() == T && std::adjacent_find(s.begin(), s.end()) == s.end(), "T %zu: not T distinct chunks", T);
        const size_t ny = std::min(nY, T / 2), nx = std::min(nX, T - ny);
        CHECK(per[0] == nx && per[1] >= ny, "T %zu stock %zu %zu: per_class %u %u, nx %zu ny %zu", T, nX, nY, per[0], per[1], nx, ny);
        CHECK((size_t)std::count(cls.begin(), cls.end(), 0) == per[0] && (size_t)std::count(cls.begin(), cls.end(), 1) == per[1], "class list and counts disagree");
        if (nX >= T - ny) {
          CHECK(per[1] == ny, "T %zu: X is long enough, yet %u chunks of Y for ny %zu", T, per[1], ny);
          for (size_t c = 1; c < T; c++) CHECK(!(cls[c] == 1 && cls[c - 1] == 1), "T %zu stock %zu %zu: two chunks of Y side by side", T, nX, nY);
        }
      }
  return n;
}

// ---- 2. the prefix rule ---------------------------------------------------------------------------------------------------------
static bool prefix_by_scan(const std::vector<uint8_t>& cls, size_t T, uint64_t w_off, uint64_t v_bytes, uint64_t w_bytes) {
  if (cls.size() < T) return false;
  for (int table = 0; table < 2; table++) {
    const uint64_t lo = table ? w_off : 0, bytes = table ? w_bytes : v_bytes;
    bool seen[3] = {false, false, false};
    size_t chunks = 0;
    for (size_t k = 0; k < T; k++) {
      const bool under = bytes ? (k * CH < lo + bytes && (k + 1) * CH > lo) : (lo / CH == k);   // chunk k holds a byte of the table
      if (under) { chunks++; seen[cls[k]] = true; }
    }
    if (chunks > 1 && !(seen[0] && seen[1])) return false;
  }
  return true;
}
static size_t check_prefix_rule(std::mt19937_64& rng) {
  size_t n = 0;
  for (int it = 0; it < 20000; it++, n++) {
    const uint64_t rs = RS[rng() % 5];
    const uint64_t w_bytes = (rng() % 8 ? 1 : 0) * 4 * ((1ull << 22) + rng() % (1ull << 28)), v_bytes = std::max<uint64_t>(w_bytes, 4) * rs / (1 + rng() % 3);
    Layout L;
    CHECK(place_layout(v_bytes, w_bytes, &L), "layout");
    std::vector<uint8_t> cls(L.T + rng() % 5 - std::min<size_t>(L.T, rng() % 8 ? 0 : 1));
    const int flavour = (int)(rng() % 4);
    for (size_t k = 0; k < cls.size(); k++) cls[k] = flavour == 0 ? (uint8_t)(k & 1) : flavour == 1 ? (uint8_t)(rng() % 3) : flavour == 2 ? (uint8_t)(rng() % 8 ? 0 : 1) : (uint8_t)(rng() % 2);
    const bool got = prefix_serves(cls, L, v_bytes, w_bytes), want = prefix_by_scan(cls, L.T, L.w_off, v_bytes, w_bytes);
    CHECK(got == want, "prefix rule: T %u v %llu w %llu: %d, by scan %d", L.T, (unsigned long long)v_bytes, (unsigned long long)w_bytes, got, want);
    if (got) {
      uint32_t per[2];
      std::vector<uint8_t> taken(cls);
      prefix_recount(&taken, L.T, per);
      CHECK(taken.size() == L.T && per[0] == (uint32_t)std::count(cls.begin(), cls.begin() + L.T, 0) && per[1] == (uint32_t)std::count(cls.begin(), cls.begin() + L.T, 1), "recount");
    }
  }
  // every prefix of length T >= 3 of an alternating list serves, where both spans cover at least two chunks
  for (size_t len = 3; len <= 40; len++)
    for (int start = 0; start < 2; start++) {
      std::vector<uint8_t> cls(len);
      for (size_t k = 0; k < len; k++) cls[k] = (uint8_t)((k + start) & 1);
      for (uint64_t v_bytes = CH + 4096; v_bytes < len * CH; v_bytes += CH / 2 + 12288)
        for (uint64_t w_bytes : {(uint64_t)1 << 20, (uint64_t)1 << 28, (uint64_t)3 << 29}) {
          Layout L;
          CHECK(place_layout(v_bytes, w_bytes, &L), "layout");
          if (L.T < 3 || L.T > len) continue;
          CHECK(prefix_serves(cls, L, v_bytes, w_bytes), "an alternating list of %zu does not serve T %u", len, L.T);
          n++;
        }
    }
  return n;
}

// ---- 3. layout and pool bound: the assertions of tests/test_place_layout.py ------------------------------------------------------
static size_t check_layout_and_bound(std::mt19937_64& rng) {
  size_t n = 0;
  for (int it = 0; it < 4000; it++, n++) {
    const uint64_t kp = KPS[rng() % 7], rows = (1ull << 20) + rng() % ((1ull << 32) - (1ull << 20));
    const uint64_t v = rows * kp * 4, w = rng() % 8 ? rows * 4 : 0;
    Layout L;
    CHECK(place_layout(v, w, &L), "layout of %llu %llu", (unsigned long long)v, (unsigned long long)w);
    const uint64_t off = L.w_off, t = L.T, w_half = ((w / 2) + 255) / 256 * 256;
    CHECK(off >= v && off % 256 == 0 && off + w <= t * CH && t * CH - (off + w) < CH + 256, "layout: w behind V, aligned, inside, no spare chunk");
    CHECK((off + w_half) % CH == 0 && off - v < CH + w, "layout: a chunk boundary in the middle of w, a gap of less than a chunk");
    const size_t T = (size_t)std::min<uint64_t>(t, 200), free_b = T * CH + ((size_t)2 << 30) + (size_t)(rng() % 300) * (CH / 2);
    const int bt = 2 + (int)(rng() % 5);
    CHECK(arena_fits(T, free_b) && !arena_fits(T, T * CH + ((size_t)2 << 30) - 1), "the arena and 2 GiB must be free");
    const size_t b = pool_bound(T, bt, free_b);
    CHECK(b >= T && b <= (size_t)bt * T + 64 && b <= std::max(T, T + (free_b / CH - T) / 2), "pool bound %zu for T %zu, %d tables, %zu free", b, T, bt, free_b / CH);
    CHECK(b == (size_t)bt * T + 64 || b == T + (free_b - T * CH) / CH / 2 || b == T, "the pool bound is one of its three terms");
  }
  Layout L;
  CHECK(!place_layout(0, 4, &L), "no V is a bad argument");
  CHECK(place_layout(400000000ull * 64, 400000000ull, &L) && L.T == 26 && L.w_off == 25 * CH - 200000000 / 256 * 256, "the bench's shape");
  return n;
}

// ---- 4. and 5. the whole sequence ---------------------------------------------------------------------------------------------------
struct Case { std::vector<int> cls_of; size_t T, max_pool, capacity; uint64_t v_bytes, w_bytes; Layout L; };
static Case make_case(std::mt19937_64& rng, size_t max_T) {
  Case c;
  do {
    const uint64_t rs = RS[rng() % 5], rows = ((2ull << 30) / (rs * 4)) + rng() % ((max_T * CH) / (rs * 4));
    c.v_bytes = rows * rs * 4; c.w_bytes = rows * 4;
    CHECK(place_layout(c.v_bytes, c.w_bytes, &c.L), "layout");
    c.T = c.L.T;
  } while (c.T > max_T);
  const size_t free_chunks = c.T + 2 + rng() % 280;
  c.max_pool = pool_bound(c.T, 2 + (int)(rng() % 5), free_chunks * CH);
  c.capacity = rng() % 3 ? SIZE_MAX : c.T + rng() % (c.max_pool - c.T + 1);    // a third of the cases: the device runs out before the bound
  const int n_cls = 2 + (int)(rng() % 3);
  const size_t max_run = RUNS[rng() % 5];
  int straddlers = (int)(rng() % 3), cur = (int)(rng() % n_cls);
  const size_t first = std::min<size_t>(8, c.max_pool);
  size_t early = 0;
  while (c.cls_of.size() < c.max_pool + 1) {
    for (size_t run = 1 + rng() % max_run; run > 0; run--) c.cls_of.push_back(cur);
    cur = (cur + 1 + (int)(rng() % (n_cls - 1))) % n_cls;
    if (straddlers > 0 && rng() % 2 && (c.cls_of.size() >= first || early + 1 < (first - 1) / 2 + 1)) {   // (the median of the first chunks stays a whole one)
      early += c.cls_of.size() < first;
      c.cls_of.push_back(-1); straddlers--;
    }
  }
  return c;
}
struct Outcome { int rc; size_t calls; };
static Outcome run_case(const Case& c, size_t fail_at, bool full_checks) {
  FakeDevice dev;
  dev.cls_of = c.cls_of; dev.capacity = c.capacity; dev.fail_at = fail_at;
  Placed out;
  const int rc = build_arena(dev, dev, c.T, c.max_pool, &out);
  const size_t T = c.T, first = std::min<size_t>(8, c.max_pool);
  if (rc != 0) {
    out = Placed();
    CHECK(dev.nothing_outstanding(), "a failed build (call %zu of kind %d failing) leaves %zu reservations, %zu mappings, %zu handles behind",
          fail_at, dev.failed_kind, dev.reservations.size(), dev.mappings.size(), dev.handles.size());
    if (!fail_at) CHECK(c.capacity <= T || c.capacity < first, "the build failed with %zu chunks for T %zu", dev.created, T);
    // a take that fails with more than T chunks in hand (and the first eight behind it) must not fail the build
    const bool in_take = dev.failed_kind == FakeDevice::CREATE || ((dev.failed_kind == FakeDevice::MAP || dev.failed_kind == FakeDevice::SET_ACCESS) && dev.failed_in_first);
    if (in_take) {
      const size_t in_hand = dev.failed_handles, index = dev.failed_kind == FakeDevice::CREATE ? in_hand : in_hand - 1;
      CHECK(!(index >= first && in_hand > T), "a take failed with %zu chunks in hand for T %zu, and the build gave up", in_hand, T);
    }
    return Outcome{rc, dev.calls};
  }
  // the arena: T chunks of 1 GiB in one reservation, and nothing else
  CHECK(out.mem.ch.size() == T && out.cls.size() == T && out.info.chunks == T && out.info.method == 2, "the arena has %zu chunks for T %zu", out.mem.ch.size(), T);
  CHECK(dev.handles.empty() && dev.mappings.size() == T && dev.reservations.size() == 1 && dev.reservations.begin()->second == T * CH,
        "after the build: %zu handles, %zu mappings, %zu reservations", dev.handles.size(), dev.mappings.size(), dev.reservations.size());
  std::vector<int> truth(T);
  for (size_t k = 0; k < T; k++) {
    CHECK(dev.mappings.count((uintptr_t)out.mem.va + k * CH), "chunk %zu of the arena is not mapped", k);
    truth[k] = c.cls_of[dev.phys_at((char*)out.mem.va + k * CH)];
  }
  if (full_checks) {
    CHECK(out.info.pool <= c.max_pool && out.info.pool >= T && dev.created <= c.max_pool, "pool %u beyond its bound %zu", out.info.pool, c.max_pool);
    for (size_t p = 0; p < dev.created; p++) {
      CHECK(dev.alone_probes[p] == (p < 8 ? 1u : 0u), "chunk %zu was timed alone %u times", p, dev.alone_probes[p]);
      if (p > 0 && c.cls_of[p] >= 0 && c.cls_of[p] == c.cls_of[p - 1]) CHECK(dev.pair_probes[p] <= 1, "chunk %zu inside a run took %u pair probes", p, dev.pair_probes[p]);
    }
    // both tables over both classes whenever what the pool held allowed it: two true classes with ceil(T/2) and floor(T/2) chunks
    std::map<int, size_t> stock;
    for (size_t p = 0; p < out.info.pool; p++) if (c.cls_of[p] >= 0) stock[c.cls_of[p]]++;
    size_t a = 0, b = 0;
    for (auto& s : stock) { if (s.second > a) { b = a; a = s.second; } else if (s.second > b) b = s.second; }
    if (a >= (T + 1) / 2 && b >= T / 2) {
      CHECK(out.info.per_class[0] == (T + 1) / 2 && out.info.per_class[1] == T / 2, "per_class %u %u for T %zu with stock %zu %zu", out.info.per_class[0], out.info.per_class[1], T, a, b);
      const size_t v_last = (c.v_bytes - 1) / CH, w_first = c.L.w_off / CH, w_last = (c.L.w_off + c.w_bytes - 1) / CH;
      for (int table = 0; table < 2; table++) {
        const size_t lo = table ? w_first : 0, hi = table ? w_last : v_last;
        std::map<int, int> under;
        for (size_t k = lo; k <= hi; k++) { CHECK(truth[k] >= 0, "a straddling chunk in an arena that needed none"); under[truth[k]]++; }
        CHECK(hi == lo || under.size() == 2, "table %d lies over %zu classes (chunks %zu .. %zu of %zu)", table, under.size(), lo, hi, T);
      }
    }
  }
  out = Placed();
  CHECK(dev.nothing_outstanding(), "releasing the arena leaves something behind");
  return Outcome{0, dev.calls};
}

// the range of a big allocation, built chunk by chunk the way fmx_dev_alloc does: complete, or nothing is left
static size_t check_big_range(std::mt19937_64& rng) {
  size_t n = 0;
  const size_t ALIGN = (size_t)2 << 20;
  for (int it = 0; it < 60; it++) {
    const size_t reserved = (((size_t)768 << 20) + rng() % ((size_t)9 << 30) + ALIGN - 1) / ALIGN * ALIGN;
    for (size_t fail_at = 0, calls = 1; fail_at <= calls; fail_at++, n++) {
      FakeDevice dev;
      dev.cls_of.assign(16, 0); dev.fail_at = fail_at;
      {
        ChunkRange R;
        bool ok = R.reserve(dev, reserved, ALIGN) == 0;
        for (size_t off = 0; off < reserved && ok; off += CH) ok = R.create(std::min(CH, reserved - off)) == 0 && R.map(R.ch.size() - 1) == 0;
        if (ok) ok = dev.set_access(R.va, reserved) == 0;
        if (!fail_at) calls = dev.calls;
        CHECK(ok == (fail_at == 0), "a big range of %zu bytes with call %zu failing: %d", reserved, fail_at, ok);
        if (ok) {
          CHECK(R.end() == reserved && dev.handles.size() == R.ch.size() && dev.mappings.size() == R.ch.size() && R.ch.size() == (reserved + CH - 1) / CH, "an incomplete range");
          ChunkRange moved(std::move(R));                                 // (what fmx_dev_free gets out of the table)
          CHECK(!R.va && R.ch.empty() && moved.release() == 0, "release");
        }
      }
      CHECK(dev.nothing_outstanding(), "a big range of %zu bytes with call %zu failing leaves something behind", reserved, fail_at);
    }
  }
  return n;
}

int main() {
  std::mt19937_64 rng(20240911);
  const size_t n_order = check_mapping_order();
  const size_t n_prefix = check_prefix_rule(rng);
  const size_t n_layout = check_layout_and_bound(rng);
  size_t n_seq = 0, n_fail = 0, n_survived = 0;
  for (int it = 0; it < 600; it++, n_seq++) {
    const Case c = make_case(rng, 40);
    (void)run_case(c, 0, true);
  }
  for (int it = 0; it < 120; it++) {
    const Case c = make_case(rng, 12);
    const Outcome whole = run_case(c, 0, true);
    for (size_t n = 1; n <= whole.calls; n++, n_fail++) n_survived += run_case(c, n, false).rc == 0;
  }
  const size_t n_big = check_big_range(rng);
  printf("place_plan_check: ok -- %zu mapping orders, %zu prefixes, %zu layouts, %zu builds, %zu builds with a failing call (%zu still succeeded), %zu big ranges\n",
         n_order, n_prefix, n_layout, n_seq, n_fail, n_survived, n_big);
  return 0;
}
