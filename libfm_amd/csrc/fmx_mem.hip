// fmx_mem.hip -- device memory of the library: fmx_dev_alloc / fmx_dev_free (fmx_internal.h), the placement of a handle's parameter
// tables (place_tables / free_tables) and the per-device arena cache.  Every decision and the owner of a chunked range are in
// fmx_place_plan.h (HIP-free, checked on the CPU by scripts/place_plan_check.cpp); this unit supplies the device.
//
// Placement of big parameter tables: an arena of chunks from two memory classes.
// scripts/ubench/placement_chunks / _order / _classes.hip (profiles/r03_placement_*.txt): the rate of random 256-byte row traffic is a
// property of the PHYSICAL memory (the same chunks mapped elsewhere keep it) and of its SPREAD: any 1 GB piece of any table runs at
// 4.9 TB/s, and so does a table whose pieces all come from one of three classes of ~96 GB the device's memory falls into; pieces of
// two classes evenly mixed run at 6.1 (3 : 1 -> 5.8, 7 : 1 -> 5.4; three classes are no better than two).  A plain allocation lies in
// one class or straddles two by luck.  build_arena (fmx_place_plan.h) takes chunks one at a time, classifies each by probing it
// together with the reference chunk of every class seen so far (k_place_pair) until two classes can supply half of the arena each,
// and maps those alternately into one range; everything else goes back.  Any failure of the virtual-memory API leaves nothing
// behind and the caller falls back to plain allocations.
#include "fmx_internal.h"
#include "fmx_place_kernels.h"
#include <atomic>

namespace {
std::atomic<uint64_t> g_devices_used{0};                              // devices fmx_create has opened a handle on in this process

// the device behind fmx_place_plan.h's two interfaces.  A failed call's error is taken off the runtime's record: it is returned.
int chk(hipError_t e) { if (e != hipSuccess) (void)hipGetLastError(); return (int)e; }
struct HipVm : Vm {
  int device = 0;
  int reserve(void** va, size_t bytes, size_t align) override { return chk(hipMemAddressReserve(va, bytes, align, nullptr, 0)); }
  int free_address(void* va, size_t bytes) override { return chk(hipMemAddressFree(va, bytes)); }
  int create(void** hnd, size_t bytes) override {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
    return chk(hipMemCreate((hipMemGenericAllocationHandle_t*)hnd, bytes, &prop, 0));
  }
  int release(void* hnd) override { return chk(hipMemRelease((hipMemGenericAllocationHandle_t)hnd)); }
  int map(void* at, size_t bytes, void* hnd) override { return chk(hipMemMap(at, bytes, 0, (hipMemGenericAllocationHandle_t)hnd, 0)); }
  int unmap(void* at, size_t bytes) override { return chk(hipMemUnmap(at, bytes)); }
  int set_access(void* at, size_t bytes) override { return access_for(at, bytes, device); }
  int access_for(void* at, size_t bytes, int dev) {
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice; acc.location.id = dev; acc.flags = hipMemAccessFlagsProtReadWrite;
    return chk(hipMemSetAccess(at, bytes, &acc, 1));
  }
};
HipVm* hip_vm(int device) {                                           // one per device, for the life of the process (ranges outlive handles)
  static HipVm* const vms = []() { HipVm* v = new HipVm[64]; for (int d = 0; d < 64; d++) v[d].device = d; return v; }();
  return (device >= 0 && device < 64) ? &vms[device] : nullptr;
}
struct HipProbe : Probe {
  fmx_handle h;
  explicit HipProbe(fmx_handle h_) : h(h_) {}
  int zero(void* at, size_t bytes) override { return chk(hipMemsetAsync(at, 0, bytes, h->stream)); }
  int sync() override { return chk(hipStreamSynchronize(h->stream)); }
  int pair_ms(void* a, void* b, float* ms) override {
    const uint32_t rows_shift = 22;                                   // 1 GiB / 256 B
    const uint32_t waves = 1u << 17;                                  // 2.1 GB of traffic per probe, ~0.4 ms
    float best = 1e30f;
    for (int rep = 0; rep < 2; rep++) {                               // (first launch: page-table warm-up; the second one is the measurement)
      hipError_t e = hipEventRecord(h->ev0, h->stream);
      hipLaunchKernelGGL(k_place_pair, dim3(waves / 4), dim3(256), 0, h->stream, (float*)a, (float*)b, rows_shift, waves, (uint64_t)rep * 7919 + 1);
      if (e == hipSuccess) e = hipGetLastError();
      if (e == hipSuccess) e = hipEventRecord(h->ev1, h->stream);
      if (e == hipSuccess) e = hipEventSynchronize(h->ev1);
      float t = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&t, h->ev0, h->ev1);
      if (e != hipSuccess) return (int)e;
      if (rep && t < best) best = t;
    }
    *ms = best;
    return 0;
  }
};

// One classified arena per device outlives its handle: the next fmx_create on that device that needs no more chunks takes it over (a
// prefix of an alternating sequence alternates) instead of probing again -- the bench's later legs, a learner's second handle.  The
// memory stays allocated until it is reused, fmx_release_cached_memory() is called, an arena_build runs short of memory, or the
// process ends (the cache is never destroyed); FMX_ARENA_CACHE=0 turns the cache off.
std::mutex g_arena_mu;
Placed* const g_arena_cache = new Placed[16];
bool arena_cache_on() { const char* e = getenv("FMX_ARENA_CACHE"); return !(e && e[0] == '0'); }
double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

void mark_device_used(int dev) { if (dev >= 0 && dev < 64) g_devices_used.fetch_or(1ull << dev, std::memory_order_relaxed); }

void arena_cache_drop(int device) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  for (int d = 0; d < 16; d++)
    if ((device < 0 || d == device) && g_arena_cache[d].mem.va) {
      int cur = 0; (void)hipGetDevice(&cur); (void)hipSetDevice(d);
      (void)g_arena_cache[d].mem.release();
      (void)hipSetDevice(cur);
    }
}

static void arena_free(fmx_handle h) {
  Placed& A = h->placed;
  if (h->device >= 0 && h->device < 16 && arena_cache_on()) {
    (void)hipStreamSynchronize(h->stream);
    std::lock_guard<std::mutex> lk(g_arena_mu);
    Placed& c = g_arena_cache[h->device];
    if (!c.mem.va || c.mem.ch.size() < A.mem.ch.size()) {            // keep the larger one
      c = std::move(A);                                               // (what the cache held is released by the assignment)
      return;
    }
  }
  const int e = A.mem.release();
  if (e) h->err = std::string("arena_free: hipMemUnmap failed: ") + hipGetErrorString((hipError_t)e);
}

// V (v_bytes) at the start of the arena, w (w_bytes) centred on a chunk boundary behind it (both classes under it too)
static bool arena_build(fmx_handle h, size_t v_bytes, size_t w_bytes, int bound_tables) {
  const auto t_start = std::chrono::steady_clock::now();
  Layout L;
  if (!place_layout(v_bytes, w_bytes, &L) || !hip_vm(h->device)) return false;
  const size_t T = L.T;
  Placed A;
  bool have = false;
  if (h->device >= 0 && h->device < 16) {                            // an arena this device's previous handle left behind?
    std::lock_guard<std::mutex> lk(g_arena_mu);
    Placed& c = g_arena_cache[h->device];
    if (c.mem.va && c.mem.ch.size() >= T) {
      if (!prefix_serves(c.cls, L, v_bytes, w_bytes)) (void)c.mem.release();     // probe again
      else {
        A = std::move(c);
        A.mem.shrink(T);                                              // the tail goes back to the device
        prefix_recount(&A.cls, T, A.info.per_class);                 // (recounted from the prefix actually taken)
        A.info.chunks = (uint32_t)T; A.info.pool = 0;                // nothing probed this time
        have = hipMemsetAsync(A.mem.va, 0, T * ARENA_CHUNK, h->stream) == hipSuccess;
        if (!have) { (void)hipGetLastError(); (void)A.mem.release(); }
      }
    }
  }
  if (!have) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    if (!arena_fits(T, free_b)) {                                     // short of memory: whatever the cache holds goes back first
      arena_cache_drop(h->device);
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    }
    if (!arena_fits(T, free_b)) return false;                         // (the caller's plain allocation reports it properly)
    HipProbe probe(h);
    A = Placed();
    if (build_arena(*hip_vm(h->device), probe, T, pool_bound(T, bound_tables, free_b), &A) != 0) return false;
  }
  h->placed = std::move(A);
  h->tb.V = (float*)h->placed.mem.va;
  h->w_sep = (float*)((char*)h->placed.mem.va + L.w_off);
  h->placed.info.seconds = since(t_start);
  return true;
}

// ---- device allocations (fmx_internal.h: fmx_dev_alloc / fmx_dev_free) -----------------------------------------------------------
namespace {
struct BigAlloc { int device = 0; ChunkRange mem; };
std::mutex g_big_mu;
auto& g_big = *new std::unordered_map<void*, BigAlloc>();            // (never destroyed: no device call at exit)
constexpr size_t BIG_MIN = (size_t)768 << 20, BIG_CHUNK = (size_t)1 << 30, BIG_ALIGN = (size_t)2 << 20;
bool big_alloc_on() { static const bool on = []() { const char* e = getenv("FMX_BIG_ALLOC"); return !(e && e[0] == '0'); }(); return on; }

hipError_t plain_alloc(void** p, size_t bytes) {          // hipMalloc; out of memory: the idle arena cache of the device goes back, once
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess) { arena_cache_drop(d); e = hipMalloc(p, bytes); }
  }
  return e;
}
// one virtual range backed by physical chunks of at most 1 GiB; false: nothing is left behind and the caller takes hipMalloc
bool big_alloc(void** p, size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || !hip_vm(dev)) return false;
  HipVm& vm = *hip_vm(dev);
  BigAlloc b; b.device = dev;
  const size_t reserved = (bytes + BIG_ALIGN - 1) / BIG_ALIGN * BIG_ALIGN;
  static const bool trace = getenv("FMX_TRACE_ALLOC") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  if (b.mem.reserve(vm, reserved, BIG_ALIGN)) return false;
  const double t_res = 1e3 * since(t0);
  bool ok = true;
  for (size_t off = 0; off < reserved && ok; off += BIG_CHUNK)
    ok = b.mem.create(std::min(BIG_CHUNK, reserved - off)) == 0 && b.mem.map(b.mem.ch.size() - 1) == 0;
  const double t_map = 1e3 * since(t0);
  if (ok) {
    // read / write for the owning device and -- where the runtime grants it -- for the OTHER DEVICES THIS PROCESS HOLDS HANDLES ON
    // (fmx_group_upload_rows copies staged rows between the devices of a one-process group); a peer the runtime refuses is not an error
    // here.  A process that drives one GPU (one process per GPU: the multi-GPU bench) never touches another device.
    int ndev = 0; (void)hipGetDeviceCount(&ndev);
    ok = vm.set_access(b.mem.va, reserved) == 0;
    const uint64_t used = g_devices_used.load(std::memory_order_relaxed);
    for (int d = 0; ok && d < ndev && d < 64; d++) {
      if (d == dev || !((used >> d) & 1ull)) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, d, dev) != hipSuccess || !can) { (void)hipGetLastError(); continue; }
      (void)vm.access_for(b.mem.va, reserved, d);
    }
  }
  if (trace) fprintf(stderr, "[fmx alloc] big %zu bytes: reserve %.3f ms, create+map %.3f ms, access %.3f ms\n", bytes, t_res, t_map - t_res, 1e3 * since(t0) - t_map);
  if (!ok) return false;                                             // (b's range releases what it holds)
  *p = b.mem.va;
  { std::lock_guard<std::mutex> lk(g_big_mu); g_big.emplace(*p, std::move(b)); }
  return true;
}
hipError_t dev_alloc_untraced(void** p, size_t bytes) {
  if (!p) return hipErrorInvalidValue;
  *p = nullptr;
  if (bytes >= BIG_MIN && big_alloc_on()) {
    if (big_alloc(p, bytes)) return hipSuccess;
    int d = 0;                                               // (out of memory next to an idle cached arena? give it back and try once more)
    if (hipGetDevice(&d) == hipSuccess) { arena_cache_drop(d); if (big_alloc(p, bytes)) return hipSuccess; }
  }
  return plain_alloc(p, bytes);
}
}  // namespace

hipError_t fmx_dev_alloc_bytes(void** p, size_t bytes) {
  static const bool trace = getenv("FMX_TRACE_ALLOC") != nullptr;
  if (!trace) return dev_alloc_untraced(p, bytes);
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = dev_alloc_untraced(p, bytes);
  const double ms = 1e3 * since(t0);
  if (ms > 0.5) fprintf(stderr, "[fmx alloc] %12zu bytes %9.3f ms%s\n", bytes, ms, e == hipSuccess ? "" : " FAILED");
  return e;
}
hipError_t fmx_dev_alloc_plain_bytes(void** p, size_t bytes) {
  if (!p) return hipErrorInvalidValue;
  *p = nullptr;
  return plain_alloc(p, bytes);
}
hipError_t fmx_dev_free(void* p) {
  if (!p) return hipSuccess;
  BigAlloc b; bool big = false;
  {
    std::lock_guard<std::mutex> lk(g_big_mu);
    auto it = g_big.find(p);
    if (it != g_big.end()) { b = std::move(it->second); g_big.erase(it); big = true; }
  }
  if (!big) return hipFree(p);
  int cur = 0; (void)hipGetDevice(&cur);
  if (cur != b.device) (void)hipSetDevice(b.device);
  (void)hipDeviceSynchronize();                              // (hipFree waits for the device's work too: nothing may still read the range)
  (void)b.mem.release();
  if (cur != b.device) (void)hipSetDevice(cur);
  return hipSuccess;
}

// ---- the tables of a handle -------------------------------------------------------------------------------------------------------
// A table of >= 256 MB is allocated up to max_tries times (the earlier candidate is held meanwhile, so that the later one is other
// memory), each candidate is zeroed and timed under a probe with the step's traffic shape, the fastest is kept (a plain allocation
// straddles two classes or not, by luck).  max_tries = 1: first fit, no probe.
static hipError_t alloc_placed(fmx_handle h, float** out, size_t bytes, int max_tries, bool rows) {
  size_t free_b = 0, total_b = 0;
  const bool probe_free = bytes >= ((size_t)256 << 20) && max_tries > 1;
  const int tries = candidate_count(bytes, max_tries, probe_free && hipMemGetInfo(&free_b, &total_b) == hipSuccess, free_b);   // candidates sit side by side
  float* cand[PLACE_MAX_CAND] = {};
  CandidateBook book;
  hipError_t er = hipSuccess;
  for (int c = 0; c < tries && er == hipSuccess; c++) {
    if (plain_alloc((void**)&cand[c], bytes) != hipSuccess) { (void)hipGetLastError(); cand[c] = nullptr; break; }
    er = hipMemsetAsync(cand[c], 0, bytes, h->stream);   // (also: a never-written allocation answers the probe in 30 us)
    if (tries == 1 || er != hipSuccess) break;
    float ms = 0.f;
    for (int rep = 0; rep < 2 && er == hipSuccess; rep++) {           // (first launch: page-table warm-up)
      er = hipEventRecord(h->ev0, h->stream);
      if (rows) {                                         // 2^19 wavefronts x 32 rows: 8 GB of traffic at k = 64, ~1.5 ms
        const uint32_t waves = 1u << 19;
        hipLaunchKernelGGL(k_place_probe, dim3(waves / 4), dim3(256), 0, h->stream, cand[c], (uint64_t)h->n_local, h->tb.rs, waves, (uint64_t)rep * 7919 + 1);
      } else {                                            // 2^24 random 4-byte read-modify-writes, ~0.5 ms
        const uint64_t total = 1ull << 24;
        hipLaunchKernelGGL(k_place_probe_w, dim3((unsigned)(total / 256)), dim3(256), 0, h->stream, cand[c], (uint64_t)(bytes / sizeof(float)), total, (uint64_t)rep * 7919 + 1);
      }
      if (er == hipSuccess) er = hipGetLastError();
      if (er == hipSuccess) er = hipEventRecord(h->ev1, h->stream);
      if (er == hipSuccess) er = hipEventSynchronize(h->ev1);
      if (er == hipSuccess) er = hipEventElapsedTime(&ms, h->ev0, h->ev1);
    }
    if (book.timed(c, ms)) break;
  }
  if (er == hipSuccess && !cand[0]) {                                    // out of memory: whatever the arena cache holds goes back first
    arena_cache_drop(h->device);
    er = plain_alloc((void**)&cand[0], bytes);                                   // (reports the allocation failure)
    if (er == hipSuccess) er = hipMemsetAsync(cand[0], 0, bytes, h->stream);
  }
  for (int c = 0; c < PLACE_MAX_CAND; c++) if ((c != book.best || er != hipSuccess) && cand[c]) { fmx_dev_free(cand[c]); cand[c] = nullptr; }
  *out = cand[book.best];
  return er;
}

// h->tb.V, h->w_sep and the report: big tables (>= 2 GiB) in an arena (arena_build); smaller ones, and every table when the
// virtual-memory API fails, as the best of up to fmx_config::place_candidates candidates (default 2)
int place_tables(fmx_handle h) {
  const auto t_place = std::chrono::steady_clock::now();
  const int pc = h->cfg.place_candidates;
  const size_t v_bytes = h->n_local * (size_t)h->tb.rs * sizeof(float), w_bytes = h->n_local * sizeof(float);
  if (pc != 1 && v_bytes >= ((size_t)2 << 30) && arena_build(h, v_bytes, w_bytes, pc > 1 ? pc : 3)) return FMX_OK;
  const int cand = pc > 0 ? std::min(pc, PLACE_MAX_CAND) : 2;
  hipError_t er = alloc_placed(h, &h->tb.V, v_bytes, cand, true);
  if (er != hipSuccess) return fail(nullptr, FMX_E_HIP, "alloc_placed(factor table) failed: %s", hipGetErrorString(er));
  er = alloc_placed(h, &h->w_sep, w_bytes, cand, false);
  if (er != hipSuccess) return fail(nullptr, FMX_E_HIP, "alloc_placed(linear weights) failed: %s", hipGetErrorString(er));
  h->placed.info.method = (cand > 1 && v_bytes >= ((size_t)256 << 20)) ? 1 : 0;
  h->placed.info.seconds = since(t_place);
  return FMX_OK;
}

void free_tables(fmx_handle h) {
  if (h->placed.mem.va) arena_free(h);                              // (both tables are parts of it)
  else { if (h->tb.V) fmx_dev_free(h->tb.V); if (h->w_sep) fmx_dev_free(h->w_sep); }
}

extern "C" {

int fmx_release_cached_memory(void) { arena_cache_drop(-1); return FMX_OK; }

// the arena of a model (fmx_place_plan.h: place_layout).  Host arithmetic, no device needed.
int fmx_place_layout(uint64_t v_bytes, uint64_t w_bytes, uint64_t* chunk_bytes, uint32_t* chunks, uint64_t* w_offset) {
  Layout L;
  if (!chunk_bytes || !chunks || !w_offset || !place_layout(v_bytes, w_bytes, &L)) return FMX_E_ARG;
  *chunk_bytes = ARENA_CHUNK; *chunks = L.T; *w_offset = L.w_off;
  return FMX_OK;
}

int fmx_get_place_info(fmx_handle h, fmx_place_info* out) {
  if (!h || !out) return FMX_E_ARG;
  *out = h->placed.info;
  return FMX_OK;
}

}  // extern "C"
