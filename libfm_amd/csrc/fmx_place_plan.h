// fmx_place_plan.h -- every host decision of device memory and table placement (fmx_mem.hip is its one user in the library), and the
// one owner of a virtual range backed by physical chunks.  Standard library only and free of HIP: the device is reached through
// the two interfaces below, so that scripts/place_plan_check.cpp can run all of it against a fake device under a sanitizer.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fmx.h"

namespace fmx {

constexpr size_t ARENA_CHUNK = (size_t)1 << 30;
constexpr int PLACE_SHORT = -1;                        // build_arena: fewer usable chunks than the arena needs (no error of the device)

// the seven calls of the virtual-memory API; 0 = success, anything else is the device's error code and is passed through
struct Vm {
  virtual int reserve(void** va, size_t bytes, size_t align) = 0;
  virtual int free_address(void* va, size_t bytes) = 0;
  virtual int create(void** hnd, size_t bytes) = 0;
  virtual int release(void* hnd) = 0;
  virtual int map(void* at, size_t bytes, void* hnd) = 0;
  virtual int unmap(void* at, size_t bytes) = 0;
  virtual int set_access(void* at, size_t bytes) = 0;
};
// what the classification does to mapped chunks: zero them, time random row traffic over two of them together (a == b: one alone)
struct Probe {
  virtual int zero(void* at, size_t bytes) = 0;
  virtual int pair_ms(void* a, void* b, float* ms) = 0;
  virtual int sync() = 0;
};

// ---- the owner: a reserved range and, per chunk, its size, its physical handle while it holds one, and whether it is mapped ------
struct ChunkRange {
  struct Chunk { size_t off = 0, size = 0; void* hnd = nullptr; bool held = false, mapped = false; };
  Vm* vm = nullptr;
  void* va = nullptr;
  size_t reserved = 0;
  std::vector<Chunk> ch;

  ChunkRange() = default;
  ChunkRange(const ChunkRange&) = delete;
  ChunkRange& operator=(const ChunkRange&) = delete;
  ChunkRange(ChunkRange&& o) noexcept { *this = std::move(o); }
  ChunkRange& operator=(ChunkRange&& o) noexcept {
    if (this != &o) { release(); vm = o.vm; va = o.va; reserved = o.reserved; ch = std::move(o.ch); o.va = nullptr; o.reserved = 0; o.ch.clear(); }
    return *this;
  }
  ~ChunkRange() { release(); }

  void* at(size_t i) const { return (char*)va + ch[i].off; }
  size_t end() const { return ch.empty() ? 0 : ch.back().off + ch.back().size; }

  int reserve(Vm& v, size_t bytes, size_t align) {
    vm = &v;
    const int e = v.reserve(&va, bytes, align);
    if (e) va = nullptr; else reserved = bytes;
    return e;
  }
  int create(size_t size) {                            // one more chunk behind the last: physical memory, not mapped yet
    void* hd = nullptr;
    const int e = vm->create(&hd, size);
    if (!e) ch.push_back(Chunk{end(), size, hd, true, false});
    return e;
  }
  int map(size_t i) {
    const int e = vm->map(at(i), ch[i].size, ch[i].hnd);
    if (!e) ch[i].mapped = true;
    return e;
  }
  // chunk i of `src` becomes this range's next chunk: unmapped there, mapped here, and counted here only after the map succeeded.
  // The handle stays with `src`, which gives it up when it is released: by then this range's mapping keeps the memory alive.
  int take_from(ChunkRange& src, size_t i) {
    Chunk& s = src.ch[i];
    int e = vm->unmap(src.at(i), s.size);
    if (e) return e;
    s.mapped = false;
    e = vm->map((char*)va + end(), s.size, s.hnd);
    if (!e) ch.push_back(Chunk{end(), s.size, nullptr, false, true});
    return e;
  }
  void shrink(size_t n) {                              // chunks [n, ..) go back to the device; the range stays reserved
    for (size_t i = n; i < ch.size(); i++) drop(ch[i]);
    if (n < ch.size()) ch.resize(n);
  }
  // unmaps exactly what is mapped (a failing unmap must not keep the other chunks), releases exactly the handles still held, frees
  // the range.  Returns the first error of an unmap.
  int release() {
    int first = 0;
    for (Chunk& c : ch) { const int e = drop(c); if (e && !first) first = e; }
    if (va) (void)vm->free_address(va, reserved);
    ch.clear(); va = nullptr; reserved = 0;
    return first;
  }

 private:
  int drop(Chunk& c) {
    const int e = c.mapped ? vm->unmap((char*)va + c.off, c.size) : 0;
    if (c.held) (void)vm->release(c.hnd);
    c.mapped = c.held = false;
    return e;
  }
};

// what a handle's tables live in: the owner (empty for methods 0 and 1) and the report; the class of every chunk (0 / 1: the two
// the tables are built from, 2: a filler) is what a later, smaller model that takes over a PREFIX recounts per_class from
struct Placed {
  ChunkRange mem;
  fmx_place_info info = {};
  std::vector<uint8_t> cls;
};

// ---- the layout: V from offset 0, w centred on the first chunk boundary behind it (half of it in either chunk: chunks alternate
// between two memory classes, so w lies in both like V does), whole chunks
struct Layout { uint64_t w_off = 0; uint32_t T = 0; };
inline bool place_layout(uint64_t v_bytes, uint64_t w_bytes, Layout* L) {
  if (v_bytes == 0) return false;
  const uint64_t CH = ARENA_CHUNK;
  const uint64_t w_half = ((w_bytes / 2) + 255) & ~(uint64_t)255;                // (256-byte granules: w stays aligned like V's rows)
  const uint64_t boundary = (v_bytes + w_half + CH - 1) / CH;                     // w straddles the start of chunk `boundary`
  L->w_off = boundary * CH - w_half;
  const uint64_t T = (L->w_off + w_bytes + CH - 1) / CH;
  if (T > 0xFFFFFFFFull) return false;
  L->T = (uint32_t)T;
  return true;
}

// ---- the pool: the arena plus 2 GiB must be free; at most bound_tables arenas' worth + 64 chunks (a class comes in runs of up to
// 64 GB in allocation order), at most half of what is free beyond the arena itself, never fewer than the arena
inline bool arena_fits(size_t T, size_t free_b) { return T * ARENA_CHUNK + ((size_t)2 << 30) <= free_b; }
inline size_t pool_bound(size_t T, int bound_tables, size_t free_b) {
  const size_t b = std::min<size_t>((size_t)bound_tables * T + 64, T + (free_b - T * ARENA_CHUNK) / ARENA_CHUNK / 2);
  return std::max<size_t>(b, T);
}

// ---- a PREFIX of a cached chunk order serves a smaller model only if it still spreads both tables over both classes: the order is a
// Bresenham spread (X X Y X Y ... for odd T or a short second class), so the prefix is recounted, never assumed to alternate
inline bool prefix_serves(const std::vector<uint8_t>& cls, const Layout& L, uint64_t v_bytes, uint64_t w_bytes) {
  const size_t T = L.T, CH = ARENA_CHUNK;
  if (cls.size() < T) return false;
  auto both = [&](size_t c0, size_t c1) {                            // chunks [c0, c1]: one chunk cannot span two classes; more must
    if (c1 <= c0) return true;
    bool s0 = false, s1 = false;
    for (size_t k = c0; k <= c1 && k < T; k++) { s0 |= cls[k] == 0; s1 |= cls[k] == 1; }
    return s0 && s1;
  };
  const size_t v_last = v_bytes ? (v_bytes - 1) / CH : 0;
  const size_t w_first = L.w_off / CH, w_last = w_bytes ? (L.w_off + w_bytes - 1) / CH : w_first;
  return both(0, v_last) && both(w_first, w_last);
}
inline void prefix_recount(std::vector<uint8_t>* cls, size_t T, uint32_t per_class[2]) {
  cls->resize(T);
  per_class[0] = per_class[1] = 0;
  for (uint8_t c : *cls) if (c < 2) per_class[c]++;
}

// ---- the class book: same class <=> two chunks together are no faster than one alone; a chunk that is faster ALONE straddles a
// border (it must not become a reference: everything would look like its class)
struct ClassBook {
  std::vector<size_t> refs;                                          // first chunk of every class
  std::vector<std::vector<size_t>> of;                               // chunks per class
  std::vector<size_t> mixed;                                         // chunks that straddle a border between classes: fillers only
  std::vector<float> alone;                                          // a chunk's time under the probe on its own (0: not timed)
  std::vector<int> cls;                                              // per chunk: its class, -1 not classified, -2 straddling
  float slow_ms = 0.f;                                               // ... of a chunk that lies in ONE class
  int last_cls = -1;

  void push() { alone.push_back(0.f); cls.push_back(-1); }
  void pop() { alone.pop_back(); cls.pop_back(); }
  void set_slow() { std::vector<float> s(alone); std::sort(s.begin(), s.end()); slow_ms = s[s.size() / 2]; }   // the median of the first chunks
  // classes come in runs of 32 / 64 chunks in allocation order: the previous chunk's class is tried first (one probe per chunk
  // inside a run), then the others in order; a chunk that matches none opens a class.  pair(ref, i, &ms) times the two together.
  template <class Pair>
  int classify(size_t i, Pair&& pair) {
    if (alone[i] > 0.f && alone[i] < 0.95f * slow_ms) { cls[i] = -2; mixed.push_back(i); return 0; }
    for (size_t t = 0; t < refs.size() && cls[i] < 0; t++) {
      const size_t k = (last_cls >= 0) ? (t == 0 ? (size_t)last_cls : (t <= (size_t)last_cls ? t - 1 : t)) : t;
      float ms = 0.f;
      const int e = pair(refs[k], i, &ms);
      if (e) return e;
      if (ms > slow_ms / 1.08f) { cls[i] = (int)k; of[k].push_back(i); last_cls = (int)k; }
    }
    if (cls[i] < 0) { refs.push_back(i); of.push_back({i}); cls[i] = (int)refs.size() - 1; last_cls = cls[i]; }
    return 0;
  }
  // the two best-stocked classes (SIZE_MAX: none); true when they hold ceil(T/2) and floor(T/2) chunks
  bool enough(size_t T, size_t* x, size_t* y) const {
    size_t a = SIZE_MAX, b = SIZE_MAX;
    for (size_t k = 0; k < of.size(); k++) {
      if (a == SIZE_MAX || of[k].size() > of[a].size()) { b = a; a = k; }
      else if (b == SIZE_MAX || of[k].size() > of[b].size()) b = k;
    }
    *x = a; *y = b;
    return a != SIZE_MAX && b != SIZE_MAX && of[a].size() >= (T + 1) / 2 && of[b].size() >= T / 2;
  }
};

// ---- the arena's chunks in mapping order: the two best-stocked classes X and Y alternately; when Y runs short (pool bound reached)
// its chunks are spread evenly among X's, then what is left of Y, the other classes and the straddling chunks (`rest`) fill up.
// cls: 0 / 1 / 2 per position; false: fewer than T chunks.
inline bool mapping_order(const std::vector<size_t>& X, const std::vector<size_t>& Y, const std::vector<size_t>& rest, size_t T,
                          std::vector<size_t>* pick, std::vector<uint8_t>* cls, uint32_t per_class[2]) {
  const size_t ny = std::min<size_t>(Y.size(), T / 2), nx = std::min<size_t>(X.size(), T - ny);
  size_t ix = 0, iy = 0, ir = 0, acc = 0;
  pick->clear(); cls->clear();
  for (size_t c = 0; c < T; c++) {
    acc += ny;
    if (iy < ny && acc >= T) { acc -= T; pick->push_back(Y[iy++]); cls->push_back(1); }
    else if (ix < nx) { pick->push_back(X[ix++]); cls->push_back(0); }
    else if (iy < Y.size()) { pick->push_back(Y[iy++]); cls->push_back(1); }
    else if (ir < rest.size()) { pick->push_back(rest[ir++]); cls->push_back(2); }
  }
  per_class[0] = (uint32_t)ix; per_class[1] = (uint32_t)iy;
  return pick->size() == T;
}
inline bool mapping_order(const ClassBook& B, size_t T, std::vector<size_t>* pick, std::vector<uint8_t>* cls, uint32_t per_class[2]) {
  size_t cx, cy;
  (void)B.enough(T, &cx, &cy);
  const std::vector<size_t> none;
  std::vector<size_t> rest;
  for (size_t k = 0; k < B.of.size(); k++) if (k != cx && k != cy) rest.insert(rest.end(), B.of[k].begin(), B.of[k].end());
  rest.insert(rest.end(), B.mixed.begin(), B.mixed.end());
  return mapping_order(cx != SIZE_MAX ? B.of[cx] : none, cy != SIZE_MAX ? B.of[cy] : none, rest, T, pick, cls, per_class);
}

// ---- the arena itself: chunks are taken one at a time into a pool's range, each is zeroed (a never-written allocation answers a
// probe in microseconds), timed on its own only while the one-class rate is being established (the first eight: a later chunk that
// straddles a border matches no reference and opens a class of its own, which never gets stocked) and classified, until two classes
// can supply half of the arena each, the pool is full, or memory runs out with more than the arena in hand.  The picked chunks move
// into a range of their own, everything else goes back.  Whatever fails, the two owners leave nothing behind.
inline int build_arena(Vm& vm, Probe& dev, size_t T, size_t max_pool, Placed* out) {
  const size_t CH = ARENA_CHUNK;
  ChunkRange P, A;
  ClassBook B;
  int er = P.reserve(vm, max_pool * CH, CH);
  if (er) return er;
  auto pair = [&](size_t i, size_t j, float* ms) { return dev.pair_ms(P.at(i), P.at(j), ms); };
  auto take = [&]() -> int {
    const size_t i = P.ch.size();
    int e = P.create(CH);
    if (e) return e;
    B.push();
    e = P.map(i);
    if (e) return e;
    e = vm.set_access(P.at(i), CH);
    if (!e) e = dev.zero(P.at(i), CH);
    if (!e && i < 8) e = pair(i, i, &B.alone[i]);
    return e;
  };
  size_t cx, cy;
  const size_t first = std::min<size_t>(8, max_pool);
  while (!er && P.ch.size() < first) er = take();
  if (!er) {
    B.set_slow();
    for (size_t i = 0; i < first && !er; i++) er = B.classify(i, pair);
  }
  while (!er && P.ch.size() < max_pool && !B.enough(T, &cx, &cy)) {
    er = take();
    if (er) {                                                         // memory ran out: go with the pool in hand
      if (P.ch.size() > T) { er = 0; if (!P.ch.back().mapped) { P.shrink(P.ch.size() - 1); B.pop(); } }
      break;
    }
    er = B.classify(P.ch.size() - 1, pair);
  }
  if (er || P.ch.size() < T) return er ? er : PLACE_SHORT;
  std::vector<size_t> pick;
  fmx_place_info info = {};
  if (!mapping_order(B, T, &pick, &out->cls, info.per_class)) return PLACE_SHORT;
  er = A.reserve(vm, T * CH, CH);
  if (er) return er;
  er = dev.sync();
  for (size_t c = 0; c < T && !er; c++) er = A.take_from(P, pick[c]);
  if (!er) er = vm.set_access(A.va, T * CH);
  if (er) return er;
  info.method = 2; info.chunks = (uint32_t)T; info.pool = (uint32_t)P.ch.size(); info.classes_seen = (uint32_t)B.refs.size();
  (void)P.release();                                                  // the unused chunks go back; the moved ones live on through their mapping
  er = dev.zero(A.va, T * CH);
  if (er) return er;
  out->mem = std::move(A);
  out->info = info;
  return 0;
}

// ---- candidates of a table of 256 MB - 2 GiB (methods 0 and 1): how many sit side by side, when to stop, which one to keep
constexpr int PLACE_MAX_CAND = 6;
inline int candidate_count(size_t bytes, int max_tries, bool free_known, size_t free_b) {
  if (bytes < ((size_t)256 << 20) || max_tries <= 1 || !free_known) return 1;
  return (int)std::min<size_t>((size_t)std::min(max_tries, PLACE_MAX_CAND), std::max<size_t>(1, free_b / (bytes + ((size_t)4 << 30))));
}
struct CandidateBook {
  float ms[PLACE_MAX_CAND] = {};
  int best = 0;
  bool timed(int c, float t) {                                        // true: two classes seen, the fast one is in hand
    ms[c] = t;
    if (ms[c] < ms[best]) best = c;
    float worst = 0.f;
    for (int i = 0; i <= c; i++) worst = std::max(worst, ms[i]);
    return c >= 1 && ms[best] < 0.95f * worst;
  }
};

}  // namespace fmx
