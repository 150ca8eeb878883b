// fmx_pipe.h -- the two-buffer pipe between device tables and a file, shared by the binary checkpoint (fmx_ckpt.hip) and the serving
// snapshot file (fmx_snap.hip).  A section is streamed in chunks through two device staging buffers and two pinned host buffers on
// h->stream: on save the pack kernel and the device-to-host copy of chunk i + 1 run while the host writes chunk i, on load the host
// reads chunk i + 1 while chunk i is copied up and unpacked.  The checksum of a section is formed on the device, by the kernel that
// moves it, over what is in device memory (fmx_ckpt_kernels.h ckpt_wave_add into Pipe::d_sum).  Internal: included by those two units only.
#pragma once
#include "fmx_internal.h"

#include <cerrno>

namespace {

// Bytes of one chunk.  Large enough that a chunk's launch, copy call and fwrite / fread call (tens of microseconds together) are
// under 1 % of the ~0.3 ms the chunk takes at PCIe rate, small enough that the four buffers (two pinned, two on the device: 64 MiB)
// cost nothing next to a model, and that a file of a few MiB still gets both buffers busy.
constexpr size_t CKPT_CHUNK = size_t(16) << 20;

struct Pipe {
  void* pin[2] = {nullptr, nullptr};
  unsigned long long* dev[2] = {nullptr, nullptr};
  hipEvent_t start[2] = {nullptr, nullptr}, end[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  unsigned long long* d_sum = nullptr;      // [0] the running checksum, [1] low word: a list's error flag
  double device_seconds = 0.0;
  hipError_t open() {
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
      e = hipHostMalloc(&pin[b], CKPT_CHUNK, hipHostMallocDefault);
      if (e == hipSuccess) e = fmx_dev_alloc(&dev[b], CKPT_CHUNK);
      if (e == hipSuccess) e = hipEventCreate(&start[b]);
      if (e == hipSuccess) e = hipEventCreate(&end[b]);
    }
    if (e == hipSuccess) e = fmx_dev_alloc(&d_sum, 16);
    return e;
  }
  // chunk b's device work is done: its pinned buffer may be read (save) or overwritten (load)
  hipError_t finish(int b) {
    if (!pending[b]) return hipSuccess;
    hipError_t e = hipEventSynchronize(end[b]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, start[b], end[b]);
    device_seconds += ms * 1e-3;
    pending[b] = false;
    return e;
  }
  ~Pipe() {
    for (int b = 0; b < 2; b++) {
      if (pin[b]) hipHostFree(pin[b]);
      fmx_dev_free(dev[b]);
      if (start[b]) hipEventDestroy(start[b]);
      if (end[b]) hipEventDestroy(end[b]);
    }
    fmx_dev_free(d_sum);
  }
};

struct File {                                // closes (and on a failed save removes) the file on every path out of a call
  FILE* f = nullptr; std::string remove_path;
  ~File() { if (f) fclose(f); if (!remove_path.empty()) remove(remove_path.c_str()); }
};

inline uint32_t stream_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 2048); }

#define CK_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(h, FMX_E_HIP, "%s: %s failed: %s", who, #expr, hipGetErrorString(_e)); } while (0)

// the stream's checksum word: zero it before a section, read it after (the stream is drained by the read)
inline int sum_reset(fmx_handle h, const char* who, Pipe& P) { CK_HIP(hipMemsetAsync(P.d_sum, 0, 16, h->stream)); return FMX_OK; }
inline int sum_read(fmx_handle h, const char* who, Pipe& P, uint64_t* sum, uint32_t* bad) {
  unsigned long long host[2] = {0ull, 0ull};
  CK_HIP(hipMemcpyAsync(host, P.d_sum, 16, hipMemcpyDeviceToHost, h->stream));
  CK_HIP(hipStreamSynchronize(h->stream));
  *sum = host[0];
  if (bad) *bad = (uint32_t)host[1];
  return FMX_OK;
}

inline double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// One section of n_units >= 1 units of unit_bytes bytes each, device -> file, `per` units to a chunk.  per * unit_bytes is a multiple
// of 8 and at most CKPT_CHUNK, so every chunk but the last ends on a word boundary.  launch(b, u0, units, word0, n_words) starts, on
// h->stream, the kernel that packs units u0 .. u0 + units - 1 into P.dev[b] -- n_words 8-byte words, the section's words word0 .. --
// and adds their checksum terms to P.d_sum.  *sum_out = the section's checksum.
template <class Launch>
int pipe_save(fmx_handle h, const char* who, Pipe& P, FILE* f, uint64_t n_units, uint64_t per, uint64_t unit_bytes, Launch launch, uint64_t* sum_out) {
  int rc = sum_reset(h, who, P); if (rc) return rc;
  uint64_t word0 = 0;
  size_t prev_bytes = 0;
  int i = 0;
  for (uint64_t u0 = 0; u0 < n_units; u0 += per, i++) {
    const int b = i & 1;
    const uint64_t units = std::min<uint64_t>(per, n_units - u0);
    const uint32_t n_words = (uint32_t)((units * unit_bytes + 7u) / 8u);
    CK_HIP(hipEventRecord(P.start[b], h->stream));
    launch(b, u0, units, word0, n_words);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpyAsync(P.pin[b], P.dev[b], (size_t)n_words * 8, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipEventRecord(P.end[b], h->stream));
    P.pending[b] = true;
    if (i > 0) {                                                 // (the host writes chunk i - 1 while the device works on chunk i)
      CK_HIP(P.finish(b ^ 1));
      if (fwrite(P.pin[b ^ 1], 1, prev_bytes, f) != prev_bytes) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
    }
    prev_bytes = (size_t)n_words * 8;
    word0 += n_words;
  }
  CK_HIP(P.finish((i - 1) & 1));
  if (fwrite(P.pin[(i - 1) & 1], 1, prev_bytes, f) != prev_bytes) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
  return sum_read(h, who, P, sum_out, nullptr);
}

// The same section, file -> device: launch unpacks P.dev[b] and adds the checksum terms of what arrived in it.
template <class Launch>
int pipe_load(fmx_handle h, const char* who, Pipe& P, FILE* f, uint64_t n_units, uint64_t per, uint64_t unit_bytes, Launch launch, uint64_t* sum_out) {
  int rc = sum_reset(h, who, P); if (rc) return rc;
  uint64_t word0 = 0;
  int i = 0;
  for (uint64_t u0 = 0; u0 < n_units; u0 += per, i++) {
    const int b = i & 1;
    const uint64_t units = std::min<uint64_t>(per, n_units - u0);
    const uint32_t n_words = (uint32_t)((units * unit_bytes + 7u) / 8u);
    CK_HIP(P.finish(b));                                         // (chunk i - 2 has left this pinned buffer; chunk i - 1 is on its way up meanwhile)
    if (fread(P.pin[b], 1, (size_t)n_words * 8, f) != (size_t)n_words * 8) return fail(h, FMX_E_ARG, "%s: read error", who);
    CK_HIP(hipEventRecord(P.start[b], h->stream));
    CK_HIP(hipMemcpyAsync(P.dev[b], P.pin[b], (size_t)n_words * 8, hipMemcpyHostToDevice, h->stream));
    launch(b, u0, units, word0, n_words);
    CK_HIP(hipGetLastError());
    CK_HIP(hipEventRecord(P.end[b], h->stream));
    P.pending[b] = true;
    word0 += n_words;
  }
  CK_HIP(P.finish(0)); CK_HIP(P.finish(1));
  return sum_read(h, who, P, sum_out, nullptr);
}

}  // namespace
