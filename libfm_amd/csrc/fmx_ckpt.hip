// fmx_ckpt.hip -- C-ABI (include/fmx.h "fmx_checkpoint_*", "fmx_group_checkpoint_*"): exact binary checkpoints of the model and of an
// open AdaGrad / FTRL session (DESIGN.md sections 24 and 28).  The byte layout and everything a load refuses from the header alone is
// fmx_ckpt_format.h (host only); the kernels are fmx_ckpt_kernels.h; the two-buffer pipe a section is streamed through, and the
// checksum formed on the device by the kernel that moves it, are fmx_pipe.h (shared with fmx_snap.hip).
//
// One save and one load serve both forms.  They work on a Team: one unsharded handle, or the members of a group with member 0 as the
// LEAD -- the file, the pipe and its two pinned buffers, the checksums and the messages are the lead's.  Only what fills or consumes a
// chunk's staging buffer knows about shards (pack_chunk / unpack_chunk), and the sparse id list (sparse_ids).
#include "fmx_pipe.h"
#include "fmx_ckpt_kernels.h"
#include "fmx_ckpt_format.h"

namespace {

namespace ck = fmx_ckpt;

struct DevBufs {                             // the sparse path's arrays, freed on every path out of a call
  uint32_t* flag = nullptr; uint32_t* pos = nullptr; uint32_t* ids = nullptr; void* tmp = nullptr;
  uint64_t count = 0;                        // flagged rows
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  ~DevBufs() { fmx_dev_free(flag); fmx_dev_free(pos); fmx_dev_free(ids); fmx_dev_free(tmp); }
};

// Who a call works on.  Everything below `ms` is used by a sharded team alone and stays empty otherwise.
struct Team {
  fmx_handle h = nullptr;                    // the lead
  std::vector<fmx_handle> ms;                // the members, the lead first ({h} for one handle)
  const char* holder = "handle";             // what a geometry message calls the model's holder
  // part[b][i]: member i's copy of chunk buffer b on ITS device.  Save: the chunk it packs (every member).  Load: where the lead's chunk
  // is copied to (members on another device than the lead's; the others read the pipe's buffer).
  // at_lead[b][i] (save): the same chunk on the lead's device -- part[b][i] itself where the member shares that device.
  std::vector<unsigned long long*> part[2], at_lead[2];
  std::vector<hipEvent_t> ev[2];             // member i is done with chunk buffer b
  hipEvent_t arrived[2] = {nullptr, nullptr};   // load: the chunk is in the pipe's buffer b
  std::vector<uint32_t*> ids;                // the file's id list on member i's device (the lead's array where the member shares its device)
  bool sharded() const { return ms.size() > 1; }
  bool with_lead(size_t i) const { return ms[i]->device == h->device; }
  Team() = default;
  Team(const Team&) = delete;
  ~Team() {
    for (int b = 0; b < 2; b++) {
      for (size_t i = 0; i < part[b].size(); i++) {
        if (i < at_lead[b].size() && at_lead[b][i] != part[b][i]) fmx_dev_free(at_lead[b][i]);
        fmx_dev_free(part[b][i]);
      }
      for (auto e : ev[b]) if (e) hipEventDestroy(e);
      if (arrived[b]) hipEventDestroy(arrived[b]);
    }
    for (size_t i = 0; i < ids.size(); i++) if (!with_lead(i)) fmx_dev_free(ids[i]);
    if (h) hipSetDevice(h->device);
  }
};

// the buffers and events of a sharded team (plain allocations: they are ends of copies between devices)
int team_open(Team& T, const char* who, bool save) {
  fmx_handle h = T.h;
  if (!T.sharded()) return FMX_OK;
  const size_t W = T.ms.size();
  T.ids.assign(W, nullptr);
  for (int b = 0; b < 2; b++) {
    T.part[b].assign(W, nullptr); T.ev[b].assign(W, nullptr);
    if (save) T.at_lead[b].assign(W, nullptr);
    for (size_t i = 0; i < W; i++) {
      CK_HIP(hipSetDevice(T.ms[i]->device));
      CK_HIP(hipEventCreateWithFlags(&T.ev[b][i], hipEventDisableTiming));
      if (save || !T.with_lead(i)) CK_HIP(fmx_dev_alloc_plain(&T.part[b][i], CKPT_CHUNK));
      if (save) T.at_lead[b][i] = T.part[b][i];
    }
    CK_HIP(hipSetDevice(h->device));
    if (save) for (size_t i = 0; i < W; i++) if (!T.with_lead(i)) { T.at_lead[b][i] = nullptr; CK_HIP(fmx_dev_alloc_plain(&T.at_lead[b][i], CKPT_CHUNK)); }
    if (!save) CK_HIP(hipEventCreateWithFlags(&T.arrived[b], hipEventDisableTiming));
  }
  return FMX_OK;
}

// rows of a chunk: as many as fit, an even number so that every chunk but the last ends on a word boundary
inline uint64_t chunk_rows(uint32_t cols) { return std::max<uint64_t>(2, (CKPT_CHUNK / ((size_t)cols * 4)) & ~size_t(1)); }

// the tables of member m behind one section of rows (ids: the sparse state's list on m's device, or nullptr)
CkptRows section_rows(fmx_handle m, uint32_t kind, uint32_t session, const uint32_t* ids) {
  CkptRows t = {nullptr, nullptr, m->tb.rs, 1u, 0u, nullptr};
  const uint32_t k = (uint32_t)m->cfg.num_factor;
  if (kind == ck::SEC_W) { t.lin = m->tb.w; t.ls = m->tb.ws; t.cols = 1; }
  else if (kind == ck::SEC_V) { t.tab = m->tb.V; t.cols = k; }
  else {
    const bool z = kind == ck::SEC_Z;
    t.tab = z ? m->ftrl.zv : session == ck::SESSION_FTRL ? m->ftrl.nv : m->adapt.nv;
    t.lin = z ? m->ftrl.zw : session == ck::SESSION_FTRL ? m->ftrl.nw : m->adapt.nw;
    t.cols = k + 1u; t.ids = ids;
  }
  return t;
}

// A sharded chunk, save: every member packs the rows it owns into a chunk of its own (0 elsewhere) on its own stream, the chunk goes
// to the lead's device where that is another one, and k_ckpt_merge on the lead's stream ORs the chunks into the pipe's buffer b and
// forms the checksum.  (The members' buffers b are free: the pipe has waited for the chunk that used them last, on the host.)
hipError_t pack_chunk(Team& T, Pipe& P, uint32_t kind, uint32_t session, int b, uint64_t r0, uint32_t n_elems, uint64_t word0, uint32_t n_words) {
  fmx_handle h = T.h;
  hipError_t e = hipSuccess;
  CkptParts parts; parts.n = (int)T.ms.size();
  for (size_t i = 0; i < T.ms.size() && e == hipSuccess; i++) {
    fmx_handle m = T.ms[i];
    e = hipSetDevice(m->device);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_ckpt_rows_shard<true>, dim3(stream_grid(n_words)), dim3(256), 0, m->stream, section_rows(m, kind, session, T.ids[i]),
                       make_shard(m->cfg), r0, n_elems, word0, T.part[b][i], (unsigned long long*)nullptr);
    e = hipGetLastError();
    if (e == hipSuccess && T.at_lead[b][i] != T.part[b][i])
      e = hipMemcpyPeerAsync(T.at_lead[b][i], h->device, T.part[b][i], m->device, (size_t)n_words * 8, m->stream);
    if (e == hipSuccess) e = hipEventRecord(T.ev[b][i], m->stream);
    parts.p[i] = T.at_lead[b][i];
  }
  const hipError_t back = hipSetDevice(h->device);
  if (e == hipSuccess) e = back;
  for (size_t i = 1; i < T.ms.size() && e == hipSuccess; i++) e = hipStreamWaitEvent(h->stream, T.ev[b][i], 0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ckpt_merge, dim3(stream_grid(n_words)), dim3(256), 0, h->stream, parts, n_words, word0, P.dev[b], P.d_sum);
  return hipGetLastError();
}

// A sharded chunk, load: the chunk is on its way into the pipe's buffer b on the lead's stream.  Every member waits for it, takes a
// copy where it sits on another device, and stores the elements it owns on its own stream; the lead's kernel also adds the checksum
// terms of all words.  The lead's stream then waits for every member, so the pipe's end event of the chunk covers them all and
// neither buffer is refilled under a reader.
hipError_t unpack_chunk(Team& T, Pipe& P, uint32_t kind, uint32_t session, int b, uint64_t r0, uint32_t n_elems, uint64_t word0, uint32_t n_words) {
  fmx_handle h = T.h;
  hipError_t e = hipEventRecord(T.arrived[b], h->stream);
  for (size_t i = 0; i < T.ms.size() && e == hipSuccess; i++) {
    fmx_handle m = T.ms[i];
    e = hipSetDevice(m->device);
    if (e == hipSuccess && i > 0) e = hipStreamWaitEvent(m->stream, T.arrived[b], 0);
    unsigned long long* src = P.dev[b];
    if (e == hipSuccess && !T.with_lead(i)) {
      src = T.part[b][i];
      e = hipMemcpyPeerAsync(src, m->device, P.dev[b], h->device, (size_t)n_words * 8, m->stream);
    }
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_ckpt_rows_shard<false>, dim3(stream_grid(n_words)), dim3(256), 0, m->stream, section_rows(m, kind, session, T.ids[i]),
                       make_shard(m->cfg), r0, n_elems, word0, src, i == 0 ? P.d_sum : (unsigned long long*)nullptr);
    e = hipGetLastError();
    if (e == hipSuccess && i > 0) e = hipEventRecord(T.ev[b][i], m->stream);
  }
  const hipError_t back = hipSetDevice(h->device);
  if (e == hipSuccess) e = back;
  for (size_t i = 1; i < T.ms.size() && e == hipSuccess; i++) e = hipStreamWaitEvent(h->stream, T.ev[b][i], 0);
  return e;
}

// one section of table rows, device -> file (fmx_pipe.h pipe_save around k_ckpt_rows / pack_chunk).  *sum_out = its checksum.
int save_rows(Team& T, const char* who, Pipe& P, FILE* f, uint32_t kind, uint32_t session, uint64_t n_rows, uint64_t* sum_out) {
  fmx_handle h = T.h;
  *sum_out = 0;
  const CkptRows t = section_rows(h, kind, session, T.ids[0]);
  if (n_rows == 0 || t.cols == 0) return FMX_OK;
  hipError_t e = hipSuccess;                                     // (of a sharded chunk: the chunks after a failed one are not started)
  const int rc = pipe_save(h, who, P, f, n_rows, chunk_rows(t.cols), (uint64_t)t.cols * 4, [&](int b, uint64_t r0, uint64_t rows, uint64_t word0, uint32_t n_words) {
    const uint32_t n_elems = (uint32_t)(rows * t.cols);
    if (!T.sharded()) hipLaunchKernelGGL(k_ckpt_rows<true>, dim3(stream_grid(n_words)), dim3(256), 0, h->stream, t, r0, n_elems, word0, P.dev[b], P.d_sum);
    else if (e == hipSuccess) e = pack_chunk(T, P, kind, session, b, r0, n_elems, word0, n_words);
  }, sum_out);
  if (e != hipSuccess) return fail(h, FMX_E_HIP, "%s: a member's share of a chunk failed: %s", who, hipGetErrorString(e));
  return rc;
}

// one section of table rows, file -> device; with ids the rows are scattered (the list has been validated).  *sum_out = the checksum
// of what arrived in the staging buffers.
int load_rows(Team& T, const char* who, Pipe& P, FILE* f, uint32_t kind, uint32_t session, uint64_t n_rows, uint64_t* sum_out) {
  fmx_handle h = T.h;
  *sum_out = 0;
  const CkptRows t = section_rows(h, kind, session, T.ids[0]);
  if (n_rows == 0 || t.cols == 0) return FMX_OK;
  hipError_t e = hipSuccess;
  const int rc = pipe_load(h, who, P, f, n_rows, chunk_rows(t.cols), (uint64_t)t.cols * 4, [&](int b, uint64_t r0, uint64_t rows, uint64_t word0, uint32_t n_words) {
    const uint32_t n_elems = (uint32_t)(rows * t.cols);
    if (!T.sharded()) hipLaunchKernelGGL(k_ckpt_rows<false>, dim3(stream_grid(n_words)), dim3(256), 0, h->stream, t, r0, n_elems, word0, P.dev[b], P.d_sum);
    else if (e == hipSuccess) e = unpack_chunk(T, P, kind, session, b, r0, n_elems, word0, n_words);
  }, sum_out);
  if (e != hipSuccess) return fail(h, FMX_E_HIP, "%s: a member's share of a chunk failed: %s", who, hipGetErrorString(e));
  return rc;
}

// the id list (padded to a multiple of 8 bytes on the device too) between the device and the file, in chunks through the pinned buffers
int copy_ids(fmx_handle h, const char* who, Pipe& P, FILE* f, uint32_t* d_ids, uint64_t count, bool to_file) {
  const uint64_t total = ck::padded(count * 4);
  int i = 0;
  size_t prev_bytes = 0;
  for (uint64_t off = 0; off < total; off += CKPT_CHUNK, i++) {
    const int b = i & 1;
    const size_t bytes = (size_t)std::min<uint64_t>(CKPT_CHUNK, total - off);
    if (!to_file) {
      CK_HIP(P.finish(b));
      if (fread(P.pin[b], 1, bytes, f) != bytes) return fail(h, FMX_E_ARG, "%s: read error", who);
    }
    CK_HIP(hipEventRecord(P.start[b], h->stream));
    if (to_file) CK_HIP(hipMemcpyAsync(P.pin[b], (const char*)d_ids + off, bytes, hipMemcpyDeviceToHost, h->stream));
    else         CK_HIP(hipMemcpyAsync((char*)d_ids + off, P.pin[b], bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipEventRecord(P.end[b], h->stream));
    P.pending[b] = true;
    if (to_file && i > 0) {
      CK_HIP(P.finish(b ^ 1));
      if (fwrite(P.pin[b ^ 1], 1, prev_bytes, f) != prev_bytes) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
    }
    prev_bytes = bytes;
  }
  CK_HIP(P.finish(0)); CK_HIP(P.finish(1));
  if (to_file && i > 0 && fwrite(P.pin[(i - 1) & 1], 1, prev_bytes, f) != prev_bytes) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
  return FMX_OK;
}

// checksum and validation of an id list that is on the device
int check_ids(fmx_handle h, const char* who, Pipe& P, const uint32_t* d_ids, uint64_t count, uint64_t* sum, uint32_t* bad) {
  *sum = 0; *bad = 0;
  if (count == 0) return FMX_OK;
  int rc = sum_reset(h, who, P); if (rc) return rc;
  hipLaunchKernelGGL(k_ckpt_ids, dim3(stream_grid((count + 1) / 2)), dim3(256), 0, h->stream, d_ids, count, (uint64_t)h->cfg.num_attribute,
                     P.d_sum, reinterpret_cast<uint32_t*>(P.d_sum + 1));
  CK_HIP(hipGetLastError());
  return sum_read(h, who, P, sum, bad);
}

// The validated id list (the lead's `ids`, padded) reaches every member: the lead's own array where the member shares its device, else
// a copy on the member's device.  Blocking: once per call.
int share_ids(Team& T, const char* who, uint32_t* ids, uint64_t count) {
  fmx_handle h = T.h;
  const size_t bytes = (size_t)std::max<uint64_t>(ck::padded(count * 4), 8);
  for (size_t i = 0; i < T.ms.size(); i++) {
    if (T.with_lead(i)) { T.ids[i] = ids; continue; }
    CK_HIP(hipSetDevice(T.ms[i]->device));
    CK_HIP(fmx_dev_alloc_plain(&T.ids[i], bytes));
    CK_HIP(hipMemcpyPeer(T.ids[i], T.ms[i]->device, ids, h->device, bytes));
  }
  CK_HIP(hipSetDevice(h->device));
  return FMX_OK;
}

uint32_t open_session(fmx_handle h) { return h->adapt.nv ? ck::SESSION_ADAGRAD : h->ftrl.nv ? ck::SESSION_FTRL : ck::SESSION_NONE; }

// flag[j] = member m's row j is not what fmx_*_begin would reproduce, over its `rows` > 0 rows, and the exclusive scan of the flags:
// launched on m's stream (m's device is current), not waited for
int flag_and_scan(fmx_handle h, const char* who, fmx_handle m, uint32_t session, uint64_t rows, DevBufs& B) {
  const int k = m->cfg.num_factor;
  CK_HIP(fmx_dev_alloc(&B.flag, rows * 4));
  CK_HIP(fmx_dev_alloc(&B.pos, rows * 4));
  const uint32_t L = (uint32_t)std::min(m->KP, 64);              // lanes per feature: a power of two
  const uint64_t waves = (rows + 64 / L - 1) / (64 / L);
  const uint32_t grid = (uint32_t)std::min<uint64_t>((waves + 3) / 4, 8192);
  if (session == ck::SESSION_ADAGRAD)
    hipLaunchKernelGGL(k_ckpt_flag_adagrad, dim3(grid), dim3(256), 0, m->stream, (const float*)m->adapt.nw, (const float*)m->adapt.nv, m->tb.rs, rows, k, L,
                       m->adapt.init_acc, B.flag);
  else
    hipLaunchKernelGGL(k_ckpt_flag_ftrl, dim3(grid), dim3(256), 0, m->stream, m->tb, (const float*)m->ftrl.zw, (const float*)m->ftrl.zv,
                       (const float*)m->ftrl.nw, (const float*)m->ftrl.nv, rows, k, L, m->ftrl.start_D(m->ftrl.l2_w), m->ftrl.l1_w,
                       m->ftrl.start_D(m->ftrl.l2_v), m->ftrl.l1_v, m->ftrl.init_acc, B.flag);
  CK_HIP(hipGetLastError());
  size_t tmp_bytes = 0;                                          // (hipcub's item count is an int: the callers bound the rows)
  CK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, B.flag, B.pos, (int)rows, m->stream));
  CK_HIP(fmx_dev_alloc_bytes(&B.tmp, std::max<size_t>(tmp_bytes, 8)));
  CK_HIP(hipcub::DeviceScan::ExclusiveSum(B.tmp, tmp_bytes, B.flag, B.pos, (int)rows, m->stream));
  return FMX_OK;
}
// ... the number of flagged rows, once the scan is done (waits for m's stream)
int flagged_count(fmx_handle h, const char* who, fmx_handle m, uint64_t rows, DevBufs& B) {
  uint32_t last[2] = {0, 0};
  CK_HIP(hipMemcpyAsync(&last[0], B.pos + (rows - 1), 4, hipMemcpyDeviceToHost, m->stream));
  CK_HIP(hipMemcpyAsync(&last[1], B.flag + (rows - 1), 4, hipMemcpyDeviceToHost, m->stream));
  CK_HIP(hipStreamSynchronize(m->stream));
  B.count = (uint64_t)last[0] + last[1];
  return FMX_OK;
}

// The sparse state's id list, ascending and padded, in D.ids on the lead's device; *state_rows = its length.  One handle: flags, their
// scan, the compaction.  Shards: every member does the same over the rows it owns, k_ckpt_global_ids turns its local rows into global
// ids, the lists meet on the lead and a radix sort there puts them in the file's order.
int sparse_ids(Team& T, const char* who, Pipe& P, uint32_t session, DevBufs& D, uint64_t* state_rows) {
  fmx_handle h = T.h;
  const uint64_t n = h->cfg.num_attribute;
  if (n > 0x7FFFFFFFull) return fail(h, FMX_E_UNSUPPORTED, "%s: the sparse state of more than 2^31 - 1 features (use FMX_CKPT_DENSE_STATE)", who);
  CK_HIP(hipEventRecord(P.start[0], h->stream));
  if (!T.sharded()) {
    int rc = flag_and_scan(h, who, h, session, n, D); if (rc) return rc;
    rc = flagged_count(h, who, h, n, D); if (rc) return rc;
    *state_rows = D.count;
    const size_t bytes = (size_t)std::max<uint64_t>(ck::padded(D.count * 4), 8);
    CK_HIP(fmx_dev_alloc(&D.ids, bytes));
    CK_HIP(hipMemsetAsync(D.ids, 0, bytes, h->stream));
    hipLaunchKernelGGL(k_ckpt_compact, dim3(stream_grid(n)), dim3(256), 0, h->stream, (const uint32_t*)D.flag, (const uint32_t*)D.pos, n, D.ids);
    CK_HIP(hipGetLastError());
  } else {
    const size_t W = T.ms.size();
    std::vector<DevBufs> B(W);
    // (every member owns n_local >= 1 rows: fmx_create refuses more shards than features)
    for (size_t i = 0; i < W; i++) {                             // every member's flags and scan are under way before any is waited for
      CK_HIP(hipSetDevice(T.ms[i]->device));
      const int rc = flag_and_scan(h, who, T.ms[i], session, T.ms[i]->n_local, B[i]); if (rc) return rc;
    }
    uint64_t total = 0;
    for (size_t i = 0; i < W; i++) {
      CK_HIP(hipSetDevice(T.ms[i]->device));
      const int rc = flagged_count(h, who, T.ms[i], T.ms[i]->n_local, B[i]); if (rc) return rc;
      total += B[i].count;
    }
    *state_rows = total;
    uint32_t* all = nullptr;                                     // the members' lists, one after the other, on the lead's device
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(fmx_dev_alloc_plain(&all, std::max<uint64_t>(total * 4, 8)));
    D.flag = all;                                                // (the lead's own flags are in B[0]: D.flag is free, and freed with D on every path out)
    uint64_t at = 0;
    for (size_t i = 0; i < W; i++) {
      fmx_handle m = T.ms[i];
      const uint64_t c = B[i].count;
      if (!c) continue;
      CK_HIP(hipSetDevice(m->device));
      CK_HIP(fmx_dev_alloc_plain(&B[i].ids, c * 4));
      hipLaunchKernelGGL(k_ckpt_compact, dim3(stream_grid(m->n_local)), dim3(256), 0, m->stream, (const uint32_t*)B[i].flag, (const uint32_t*)B[i].pos,
                         m->n_local, B[i].ids);
      CK_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_ckpt_global_ids, dim3(stream_grid(c)), dim3(256), 0, m->stream, make_shard(m->cfg), B[i].ids, c);
      CK_HIP(hipGetLastError());
      CK_HIP(hipMemcpyPeerAsync(all + at, h->device, B[i].ids, m->device, c * 4, m->stream));
      at += c;
    }
    for (size_t i = 0; i < W; i++) if (B[i].count) { CK_HIP(hipSetDevice(T.ms[i]->device)); CK_HIP(hipStreamSynchronize(T.ms[i]->stream)); }
    CK_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)std::max<uint64_t>(ck::padded(total * 4), 8);
    CK_HIP(fmx_dev_alloc_plain(&D.ids, bytes));
    CK_HIP(hipMemsetAsync(D.ids, 0, bytes, h->stream));
    if (total) {
      size_t tmp_bytes = 0;
      CK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const uint32_t*)all, D.ids, (int)total, 0, 32, h->stream));
      CK_HIP(fmx_dev_alloc_bytes(&D.tmp, std::max<size_t>(tmp_bytes, 8)));
      CK_HIP(hipcub::DeviceRadixSort::SortKeys(D.tmp, tmp_bytes, (const uint32_t*)all, D.ids, (int)total, 0, 32, h->stream));
    }
    CK_HIP(hipStreamSynchronize(h->stream));                     // (B's arrays and the sort's input go out of use here)
  }
  CK_HIP(hipEventRecord(P.end[0], h->stream));
  P.pending[0] = true;
  CK_HIP(P.finish(0));
  return FMX_OK;
}

// what both entry points of one handle refuse from their arguments and the handle's kind
int ckpt_check(fmx_handle h, const char* who, const char* path, const fmx_ckpt_opts* opts, uint32_t* flags) {
  if (!path) return fail(h, FMX_E_ARG, "%s: path is NULL", who);
  *flags = opts ? opts->flags : 0u;
  if (*flags & ~ck::KNOWN_FLAGS) return fail(h, FMX_E_ARG, "%s: unknown flags 0x%x", who, *flags);
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  return FMX_OK;
}

// ... and of a group whose members are all there (nothing launched, nothing changed): the members' kinds and the same two arguments.
// The messages are on the lead.
int group_ckpt_check(fmx_group g, const char* who, const char* path, const fmx_ckpt_opts* opts, uint32_t* flags) {
  fmx_handle h = g->hs[0];
  for (auto m : g->hs) { const int sr = serve_refuse(m, who); if (sr) { h->err = m->err; return sr; } }
  for (auto m : g->hs) if (m->comm) return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on communicator ranks (fmx_comm_init_rank)", who);
  if (!path) return fail(h, FMX_E_ARG, "%s: path is NULL", who);
  *flags = opts ? opts->flags : 0u;
  if (*flags & ~ck::KNOWN_FLAGS) return fail(h, FMX_E_ARG, "%s: unknown flags 0x%x", who, *flags);
  for (size_t i = 1; i < g->hs.size(); i++) {
    fmx_handle m = g->hs[i];
    if (m->cfg.num_factor != h->cfg.num_factor || (m->cfg.k0 != 0) != (h->cfg.k0 != 0) || (m->cfg.k1 != 0) != (h->cfg.k1 != 0))
      return fail(h, FMX_E_STATE, "%s: shard %zu describes another model than shard 0 (num_factor, k0, k1)", who, i);
    if (open_session(m) != open_session(h))
      return fail(h, FMX_E_STATE, "%s: shard %zu holds another kind of AdaGrad / FTRL session than shard 0", who, i);
  }
  return FMX_OK;
}

void fill_info(fmx_ckpt_info* info, const ck::Header& hd, uint64_t bytes, double seconds, double device_seconds) {
  if (!info) return;
  memset(info, 0, sizeof(*info));
  info->version = hd.version; info->session = hd.session; info->num_attribute = hd.num_attribute; info->num_factor = hd.num_factor;
  info->k0 = hd.k0; info->k1 = hd.k1; info->flags = hd.flags; info->state_rows = hd.state_rows; info->bytes = bytes;
  info->seconds = seconds; info->device_seconds = device_seconds;
}

// read the header of an open file; *file_len = the file's length
bool read_header(FILE* f, ck::Header* hd, uint64_t* file_len, char* err, size_t err_len) {
  uint8_t buf[ck::HEADER_BYTES];
  if (fseeko(f, 0, SEEK_END) != 0) { snprintf(err, err_len, "cannot seek"); return false; }
  const off_t len = ftello(f);
  if (len < 0 || fseeko(f, 0, SEEK_SET) != 0) { snprintf(err, err_len, "cannot seek"); return false; }
  *file_len = (uint64_t)len;
  const size_t got = fread(buf, 1, sizeof(buf), f);
  return ck::parse(buf, got, *file_len, hd, err, err_len);
}

// every member's own stream is drained and its model up to date; the lead's device is current afterwards
int team_settle(Team& T) {
  fmx_handle h = T.h;
  for (auto m : T.ms) {
    { int _rc = lag_flush(m); if (_rc) { if (m != h) h->err = m->err; return _rc; } }
    HIPCHK(h, hipSetDevice(m->device));
    HIPCHK(h, hipStreamSynchronize(m->stream));
  }
  HIPCHK(h, hipSetDevice(h->device));
  return FMX_OK;
}

// fmx_checkpoint_save / fmx_group_checkpoint_save behind their checks
int save_impl(Team& T, const char* who, const char* path, uint32_t flags, fmx_ckpt_info* info) {
  fmx_handle h = T.h;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = team_settle(T); if (rc) return rc;
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;

  ck::Header hd;
  hd.session = (flags & ck::FLAG_MODEL_ONLY) ? ck::SESSION_NONE : open_session(h);
  hd.num_attribute = n; hd.num_factor = (uint32_t)k; hd.k0 = h->cfg.k0 ? 1u : 0u; hd.k1 = h->cfg.k1 ? 1u : 0u;
  hd.flags = flags;
  const bool dense = (flags & ck::FLAG_DENSE) != 0;
  if (hd.session == ck::SESSION_ADAGRAD) { hd.consts[0] = h->adapt.eta; hd.consts[1] = h->adapt.init_acc; }
  if (hd.session == ck::SESSION_FTRL) {
    const FtrlState& f = h->ftrl;
    const float c[7] = {f.inv_alpha, f.beta, f.l1_w, f.l1_v, f.l2_w, f.l2_v, f.init_acc};
    memcpy(hd.consts, c, sizeof(c));
  }

  Pipe P;
  DevBufs D;
  CK_HIP(P.open());
  rc = team_open(T, who, true); if (rc) return rc;
  if (!T.sharded()) T.ids.assign(1, nullptr);
  // the sparse path first, so that the plan of the file is complete before its first byte
  if (hd.session != ck::SESSION_NONE && dense) hd.state_rows = n;
  if (hd.session != ck::SESSION_NONE && !dense) { rc = sparse_ids(T, who, P, hd.session, D, &hd.state_rows); if (rc) return rc; }
  const uint64_t total = ck::plan(&hd);

  File F;
  const std::string tmp_path = std::string(path) + ".tmp";
  F.f = fopen(tmp_path.c_str(), "wb");
  if (!F.f) return fail(h, FMX_E_ARG, "%s: cannot create %s (%s)", who, tmp_path.c_str(), strerror(errno));
  F.remove_path = tmp_path;
  uint8_t head[ck::HEADER_BYTES];
  memset(head, 0, sizeof(head));                                 // (the header is written again, with the checksums, at the end)
  if (fwrite(head, 1, sizeof(head), F.f) != sizeof(head)) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));

  for (uint32_t si = 0; si < hd.n_sections; si++) {
    ck::Section& s = hd.sec[si];
    if (s.kind == ck::SEC_W0) {                                  // (replicated: the lead's)
      uint8_t b[8];
      double w0 = 0.0;
      CK_HIP(hipMemcpy(&w0, h->w0, sizeof(double), hipMemcpyDeviceToHost));
      uint64_t u; memcpy(&u, &w0, 8); ck::put_u64(b, u);
      s.checksum = ck::checksum(b, 8);
      if (fwrite(b, 1, 8, F.f) != 8) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
    } else if (s.kind == ck::SEC_IDS) {
      uint32_t bad = 0;
      rc = check_ids(h, who, P, D.ids, hd.state_rows, &s.checksum, &bad); if (rc) return rc;
      if (bad) return fail(h, FMX_E_HIP, "%s: the id list built on the device is not ascending", who);
      rc = copy_ids(h, who, P, F.f, D.ids, hd.state_rows, true); if (rc) return rc;
      if (T.sharded()) { rc = share_ids(T, who, D.ids, hd.state_rows); if (rc) return rc; }
      else T.ids[0] = D.ids;
    } else {
      const bool state = s.kind != ck::SEC_W && s.kind != ck::SEC_V;
      rc = save_rows(T, who, P, F.f, s.kind, hd.session, state ? hd.state_rows : n, &s.checksum); if (rc) return rc;
    }
  }
  if ((uint64_t)ftello(F.f) != total) return fail(h, FMX_E_ARG, "%s: wrote %lld bytes where the plan has %llu", who, (long long)ftello(F.f), (unsigned long long)total);
  ck::encode(hd, head);
  if (fseeko(F.f, 0, SEEK_SET) != 0 || fwrite(head, 1, sizeof(head), F.f) != sizeof(head) || fflush(F.f) != 0)
    return fail(h, FMX_E_ARG, "%s: write error on %s (%s)", who, tmp_path.c_str(), strerror(errno));
  const int cl = fclose(F.f);
  F.f = nullptr;
  if (cl != 0) return fail(h, FMX_E_ARG, "%s: write error on %s (%s)", who, tmp_path.c_str(), strerror(errno));
  if (rename(tmp_path.c_str(), path) != 0) return fail(h, FMX_E_ARG, "%s: cannot rename %s to %s (%s)", who, tmp_path.c_str(), path, strerror(errno));
  F.remove_path.clear();
  fill_info(info, hd, total, since(t0), P.device_seconds);
  return FMX_OK;
}

// fmx_checkpoint_load / fmx_group_checkpoint_load behind the checks of their arguments
int load_impl(Team& T, const char* who, const char* path, uint32_t flags, fmx_ckpt_info* info) {
  fmx_handle h = T.h;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < T.ms.size(); i++) {
    char where[32] = "";
    if (T.sharded()) snprintf(where, sizeof(where), " on shard %zu", i);
    if (T.ms[i]->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open%s (call fmx_sgda_end first)", who, where);
    if (T.ms[i]->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open%s (call fmx_als_end first)", who, where);
  }
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) return fail(h, FMX_E_ARG, "%s: cannot open %s (%s)", who, path, strerror(errno));
  ck::Header hd;
  uint64_t file_len = 0;
  char err[256] = "";
  if (!read_header(F.f, &hd, &file_len, err, sizeof(err))) return fail(h, FMX_E_ARG, "%s: %s: %s", who, path, err);
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  if (hd.num_attribute != n) return fail(h, FMX_E_ARG, "%s: num_attribute is %llu in the file and %llu on the %s", who, (unsigned long long)hd.num_attribute, (unsigned long long)n, T.holder);
  if (hd.num_factor != (uint32_t)k) return fail(h, FMX_E_ARG, "%s: num_factor is %u in the file and %d on the %s", who, hd.num_factor, k, T.holder);
  if (hd.k0 != (h->cfg.k0 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k0 is %u in the file and %d on the %s", who, hd.k0, h->cfg.k0 ? 1 : 0, T.holder);
  if (hd.k1 != (h->cfg.k1 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k1 is %u in the file and %d on the %s", who, hd.k1, h->cfg.k1 ? 1 : 0, T.holder);
  const bool take_session = hd.session != ck::SESSION_NONE && !(flags & ck::FLAG_MODEL_ONLY);
  AdaptState as; FtrlState fs;
  if (take_session && hd.session == ck::SESSION_ADAGRAD) {
    as.eta = hd.consts[0]; as.init_acc = hd.consts[1];
    if (!(as.eta >= 0.f) || std::isinf(as.eta) || !(as.init_acc > 0.f) || std::isinf(as.init_acc))
      return fail(h, FMX_E_ARG, "%s: the file's AdaGrad constants (eta %g, init_acc %g) are not ones fmx_adapt_begin sets", who, (double)as.eta, (double)as.init_acc);
  }
  if (take_session && hd.session == ck::SESSION_FTRL) {
    fs.inv_alpha = hd.consts[0]; fs.beta = hd.consts[1]; fs.l1_w = hd.consts[2]; fs.l1_v = hd.consts[3]; fs.l2_w = hd.consts[4];
    fs.l2_v = hd.consts[5]; fs.init_acc = hd.consts[6];
    bool ok = fs.inv_alpha > 0.f && fs.start_D(fs.l2_w) > 0.f && fs.start_D(fs.l2_v) > 0.f && !std::isinf(fs.start_D(fs.l2_w)) && !std::isinf(fs.start_D(fs.l2_v));
    for (int i = 1; i < 7; i++) ok = ok && hd.consts[i] >= 0.f && !std::isinf(hd.consts[i]);
    if (!ok) return fail(h, FMX_E_ARG, "%s: the file's FTRL constants are not ones fmx_ftrl_begin sets", who);
  }
  // ---- nothing has changed up to here; from here on a failure leaves the parameters unspecified and closes the session ----
  for (auto m : T.ms) touch_w(m);
  int rc = team_settle(T); if (rc) return rc;
  Pipe P;
  DevBufs D;
  CK_HIP(P.open());
  auto broken = [&](int code, const char* what, const char* section) {
    const std::string before = code == FMX_E_ARG ? std::string() : h->err;    // (a HIP or read error keeps its own text in front)
    for (auto m : T.ms) {                                                      // (every member's session: all or none)
      hipSetDevice(m->device);
      if (m->stream) hipStreamSynchronize(m->stream);
      adapt_free(m); ftrl_free(m);
    }
    hipSetDevice(h->device);
    return fail(h, code, "%s: %s%s%s in section '%s' of %s: the parameters are unspecified and any AdaGrad / FTRL session has been closed",
                who, before.c_str(), before.empty() ? "" : "; ", what, section, path);
  };
  rc = team_open(T, who, false); if (rc) return broken(rc, "no memory for the members' buffers", "w0");
  if (!T.sharded()) T.ids.assign(1, nullptr);
  bool session_ready = false;
  for (uint32_t si = 0; si < hd.n_sections; si++) {
    const ck::Section& s = hd.sec[si];
    const char* name = ck::section_name(s.kind);
    if (s.kind >= ck::SEC_IDS && !take_session) break;           // (the rest of the file is the session)
    if (s.kind >= ck::SEC_IDS && !session_ready) {
      session_ready = true;
      // the first section of the session: the parameters are in place, so its tables and their start state come first, on every member
      for (auto m : T.ms) {
        if (hipSetDevice(m->device) != hipSuccess) return broken(FMX_E_HIP, "hipSetDevice failed", name);
        if (hd.session == ck::SESSION_ADAGRAD) {
          if (m->ftrl.nv) ftrl_free(m);
          rc = adapt_tables(m, who);
          if (rc) { if (m != h) h->err = m->err; return broken(rc, "no memory for the session", name); }
          m->adapt.eta = as.eta; m->adapt.init_acc = as.init_acc;
          rc = adapt_start_state(m);
        } else {
          if (m->adapt.nv) adapt_free(m);
          rc = ftrl_tables(m, who);
          if (rc) { if (m != h) h->err = m->err; return broken(rc, "no memory for the session", name); }
          FtrlState f = fs;
          f.zw = m->ftrl.zw; f.zv = m->ftrl.zv; f.nw = m->ftrl.nw; f.nv = m->ftrl.nv;
          m->ftrl = f;
          rc = ftrl_start_state(m);
        }
        if (rc) { if (m != h) h->err = m->err; return broken(rc, "the start state failed", name); }
      }
      if (hipSetDevice(h->device) != hipSuccess) return broken(FMX_E_HIP, "hipSetDevice failed", name);
    }
    if (fseeko(F.f, (off_t)s.offset, SEEK_SET) != 0) return broken(FMX_E_ARG, "cannot seek", name);
    uint64_t sum = 0;
    if (s.kind == ck::SEC_W0) {
      uint8_t b[8];
      if (fread(b, 1, 8, F.f) != 8) return broken(FMX_E_ARG, "read error", name);
      sum = ck::checksum(b, 8);
      if (sum == s.checksum) {
        const uint64_t u = ck::get_u64(b);
        double w0; memcpy(&w0, &u, 8);
        for (auto m : T.ms)                                      // (replicated: every member's)
          if (hipSetDevice(m->device) != hipSuccess || hipMemcpy(m->w0, &w0, sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return broken(FMX_E_HIP, "device copy failed", name);
        if (hipSetDevice(h->device) != hipSuccess) return broken(FMX_E_HIP, "hipSetDevice failed", name);
      }
    } else if (s.kind == ck::SEC_IDS) {
      // the whole list is validated on the lead, and the flag read back, before it reaches a member and before any row is scattered
      // (sharded: a plain allocation, the source of copies to the members' devices)
      const size_t id_bytes = (size_t)std::max<uint64_t>(ck::padded(hd.state_rows * 4), 8);
      if ((T.sharded() ? fmx_dev_alloc_plain(&D.ids, id_bytes) : fmx_dev_alloc(&D.ids, id_bytes)) != hipSuccess) return broken(FMX_E_HIP, "no memory for the id list", name);
      rc = copy_ids(h, who, P, F.f, D.ids, hd.state_rows, false); if (rc) return broken(rc, "stream error", name);
      uint32_t bad = 0;
      rc = check_ids(h, who, P, D.ids, hd.state_rows, &sum, &bad); if (rc) return broken(rc, "stream error", name);
      if (bad) return broken(FMX_E_ARG, "ids that are not strictly ascending or not below num_attribute", name);
      if (sum == s.checksum) {
        if (T.sharded()) { rc = share_ids(T, who, D.ids, hd.state_rows); if (rc) return broken(rc, "stream error", name); }
        else T.ids[0] = D.ids;
      }
    } else {
      const bool state = s.kind != ck::SEC_W && s.kind != ck::SEC_V;
      rc = load_rows(T, who, P, F.f, s.kind, hd.session, state ? hd.state_rows : n, &sum); if (rc) return broken(rc, "stream error", name);
    }
    if (sum != s.checksum) return broken(FMX_E_ARG, "checksum mismatch", name);
  }
  rc = team_settle(T); if (rc) return rc;
  fill_info(info, hd, file_len, since(t0), P.device_seconds);
  return FMX_OK;
}

}  // namespace

extern "C" {

int fmx_checkpoint_save(fmx_handle h, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_checkpoint_save";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, who); if (_sr) return _sr; }
  uint32_t flags = 0;
  const int rc = ckpt_check(h, who, path, opts, &flags); if (rc) return rc;
  Team T; T.h = h; T.ms.assign(1, h);
  return save_impl(T, who, path, flags, info);
}

int fmx_checkpoint_load(fmx_handle h, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_checkpoint_load";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, who); if (_sr) return _sr; }
  uint32_t flags = 0;
  const int rc = ckpt_check(h, who, path, opts, &flags); if (rc) return rc;
  Team T; T.h = h; T.ms.assign(1, h);
  return load_impl(T, who, path, flags, info);
}

// The group forms.  A group of one unsharded handle is a team of one: the per-handle call's own path, bits and bytes.
int fmx_group_checkpoint_save(fmx_group g, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_group_checkpoint_save";
  if (!g) return FMX_E_ARG;
  for (auto m : g->hs) if (!m) { g->err = "a member of the group was destroyed"; return FMX_E_STATE; }
  uint32_t flags = 0;
  int rc = group_ckpt_check(g, who, path, opts, &flags);
  if (rc == FMX_OK) {
    Team T; T.h = g->hs[0]; T.ms = g->hs; T.holder = "group";
    rc = save_impl(T, who, path, flags, info);
  }
  if (rc) g->err = g->hs[0]->err;
  return rc;
}

int fmx_group_checkpoint_load(fmx_group g, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_group_checkpoint_load";
  if (!g) return FMX_E_ARG;
  for (auto m : g->hs) if (!m) { g->err = "a member of the group was destroyed"; return FMX_E_STATE; }
  uint32_t flags = 0;
  int rc = group_ckpt_check(g, who, path, opts, &flags);
  if (rc == FMX_OK) {
    Team T; T.h = g->hs[0]; T.ms = g->hs; T.holder = "group";
    rc = load_impl(T, who, path, flags, info);
  }
  if (rc) g->err = g->hs[0]->err;
  return rc;
}

int fmx_checkpoint_info(const char* path, fmx_ckpt_info* info, char* err, size_t err_len) {
  char local[256] = "";
  auto say = [&](const char* text) { if (err && err_len) snprintf(err, err_len, "%s", text); return FMX_E_ARG; };
  if (!path || !info) return say("fmx_checkpoint_info: path or info is NULL");
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) { snprintf(local, sizeof(local), "cannot open %s (%s)", path, strerror(errno)); return say(local); }
  ck::Header hd;
  uint64_t file_len = 0;
  if (!read_header(F.f, &hd, &file_len, local, sizeof(local))) return say(local);
  fill_info(info, hd, file_len, 0.0, 0.0);
  return FMX_OK;
}

}  // extern "C"
