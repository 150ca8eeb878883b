// fmx_snap.hip -- C-ABI (include/fmx.h "fmx_compact_save" ... "fmx_serve_open"): the serving snapshot as a file, and the serve-only
// handle that holds such a file's snapshot and no model.  The byte layout and everything a load refuses from the
// header alone is fmx_snap_format.h (host only); the kernels are fmx_snap_kernels.h; the two-buffer pipe a section is streamed through
// is fmx_pipe.h, shared with the checkpoint.  A save reads the snapshot's device tables and nothing else.  A load builds the new
// snapshot BESIDE the handle's, from plain allocations like compact_build's and for its reason, and swaps it in only after every
// section's checksum -- over what arrived in device memory -- has matched and a pruned file's directory has been validated on the
// device (k_snap_dir_check): a failure leaves the handle's snapshot and model exactly as they were.
#include "fmx_pipe.h"
#include "fmx_snap_kernels.h"
#include "fmx_snap_format.h"

namespace {

namespace sn = fmx_snap;

// units of a chunk: as many as fit, a multiple of 4, so that every chunk but the last ends on a word boundary whatever the unit (a bf16
// row of num_factor u16 is the narrowest: 2 * num_factor bytes)
inline uint64_t chunk_units(uint64_t unit_bytes) { return std::max<uint64_t>(4, (CKPT_CHUNK / unit_bytes) & ~uint64_t(3)); }

// one section between a snapshot table (rows of `cols` elements of T, rs apart) and the file.  TO_FILE: device -> file, else file -> device
template <class T, bool TO_FILE>
int stream_table(fmx_handle h, const char* who, Pipe& P, FILE* f, T* tab, uint32_t rs, uint32_t cols, uint64_t n_rows, uint64_t* sum_out) {
  *sum_out = 0;
  if (n_rows == 0 || cols == 0) return FMX_OK;
  const uint64_t unit = (uint64_t)cols * sizeof(T);
  auto launch = [&](int b, uint64_t r0, uint64_t rows, uint64_t word0, uint32_t n_words) {
    hipLaunchKernelGGL((k_snap_rows<T, TO_FILE>), dim3(stream_grid(n_words)), dim3(256), 0, h->stream, tab, rs, cols, r0, (uint32_t)(rows * cols), word0,
                       P.dev[b], P.d_sum);
  };
  if (TO_FILE) return pipe_save(h, who, P, f, n_rows, chunk_units(unit), unit, launch, sum_out);
  return pipe_load(h, who, P, f, n_rows, chunk_units(unit), unit, launch, sum_out);
}

// a section of the snapshot `c` by its kind (rs: the handle's row stride)
template <bool TO_FILE>
int stream_section(fmx_handle h, const char* who, Pipe& P, FILE* f, const CompactState& c, uint32_t rs, uint32_t kind, const sn::Header& hd, uint64_t* sum) {
  typedef unsigned long long u64;
  const uint64_t rows = sn::rows_of(hd);
  switch (kind) {
    case sn::SEC_DIR:  return stream_table<u64, TO_FILE>(h, who, P, f, reinterpret_cast<u64*>(c.dir), 1u, 1u, (hd.num_attribute + 31) / 32, sum);
    case sn::SEC_ROWS: return stream_table<u64, TO_FILE>(h, who, P, f, reinterpret_cast<u64*>(c.B), 1u, 1u, rows * (uint64_t)(hd.P / 8u), sum);
    case sn::SEC_W:    return stream_table<uint32_t, TO_FILE>(h, who, P, f, reinterpret_cast<uint32_t*>(c.w), 1u, 1u, rows, sum);
    case sn::SEC_V:    return stream_table<uint16_t, TO_FILE>(h, who, P, f, c.V, rs, hd.num_factor, rows, sum);
    default:           return fail(h, FMX_E_ARG, "%s: unknown section kind %u", who, kind);
  }
}

// what the handle-bound entry points refuse from their arguments and the handle's kind
int snap_check(fmx_handle h, const char* who, const char* path) {
  if (!path) return fail(h, FMX_E_ARG, "%s: path is NULL", who);
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
  return FMX_OK;
}

uint64_t device_bytes(const sn::Header& hd, uint32_t rs) {
  const uint64_t rows = sn::rows_of(hd);
  return (hd.format == sn::FORMAT_INT8 ? rows * (uint64_t)hd.P : rows * (2 * (uint64_t)rs + 4)) + (hd.pruned ? (hd.num_attribute + 31) / 32 * 8 : 0);
}

// bytes_compact: the snapshot's device bytes on a handle with row stride rs (0: no handle, fmx_snapshot_info)
void fill_info(fmx_snap_info* info, const sn::Header& hd, uint64_t bytes, uint64_t bytes_compact, double seconds, double device_seconds) {
  if (!info) return;
  memset(info, 0, sizeof(*info));
  info->version = hd.version; info->format = hd.format; info->num_attribute = hd.num_attribute; info->num_factor = hd.num_factor;
  info->k0 = hd.k0; info->k1 = hd.k1; info->task = (int32_t)hd.task; info->min_target = hd.min_target; info->max_target = hd.max_target;
  info->pruned = hd.pruned; info->row_bytes = hd.P; info->kept = hd.kept; info->rows = sn::rows_of(hd);
  info->nonfinite = hd.nonfinite; info->max_abs_err = hd.max_abs_err; info->sum_sq_err = hd.sum_sq_err;
  info->dropped_dead = hd.dropped_dead; info->dropped_unseen = hd.dropped_unseen;
  info->bytes = bytes; info->bytes_compact = bytes_compact; info->seconds = seconds; info->device_seconds = device_seconds;
}

// read the header of an open file; *file_len = the file's length
bool read_header(FILE* f, sn::Header* hd, uint64_t* file_len, char* err, size_t err_len) {
  uint8_t buf[sn::HEADER_BYTES];
  if (fseeko(f, 0, SEEK_END) != 0) { snprintf(err, err_len, "cannot seek"); return false; }
  const off_t len = ftello(f);
  if (len < 0 || fseeko(f, 0, SEEK_SET) != 0) { snprintf(err, err_len, "cannot seek"); return false; }
  *file_len = (uint64_t)len;
  const size_t got = fread(buf, 1, sizeof(buf), f);
  return sn::parse(buf, got, *file_len, hd, err, err_len);
}

// fmx_compact_load behind its argument checks, for fmx_serve_open too: F is open, hd its parsed header
int load_into(fmx_handle h, const char* who, const char* path, File& F, const sn::Header& hd, uint64_t file_len, fmx_snap_info* info) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  if (hd.num_attribute != n) return fail(h, FMX_E_ARG, "%s: num_attribute is %llu in the file and %llu on the handle", who, (unsigned long long)hd.num_attribute, (unsigned long long)n);
  if (hd.num_factor != (uint32_t)k) return fail(h, FMX_E_ARG, "%s: num_factor is %u in the file and %d on the handle", who, hd.num_factor, k);
  if (hd.k0 != (h->cfg.k0 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k0 is %u in the file and %d on the handle", who, hd.k0, h->cfg.k0 ? 1 : 0);
  if (hd.k1 != (h->cfg.k1 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k1 is %u in the file and %d on the handle", who, hd.k1, h->cfg.k1 ? 1 : 0);
  HIPCHK(h, hipSetDevice(h->device));
  const uint32_t rs = h->tb.rs;
  const bool i8 = hd.format == sn::FORMAT_INT8;
  const uint64_t rows = sn::rows_of(hd), nwords = (n + 31) / 32;
  const size_t arows = (size_t)std::max<uint64_t>(rows, 1);       // (a pruned snapshot that keeps nothing still gets tables of one row, as compact_build's)
  Pipe P;
  CompactState c;
  // everything below leaves through `out`: the stream drained, the new tables freed unless they were handed to the handle
  auto out = [&](int rc) { if (h->stream) hipStreamSynchronize(h->stream); compact_release(c); return rc; };
  auto broken = [&](int code, const char* what, const char* section) {
    const std::string before = code == FMX_E_ARG ? std::string() : h->err;    // (a HIP or read error keeps its own text in front)
    return out(fail(h, code, "%s: %s%s%s in section '%s' of %s: nothing was loaded, the handle's own snapshot (if any) is unchanged",
                    who, before.c_str(), before.empty() ? "" : "; ", what, section, path));
  };
  c.format = hd.format; c.kept = hd.pruned ? hd.kept : 0;
  c.nonfinite = hd.nonfinite; c.max_abs_err = hd.max_abs_err; c.sum_sq_err = hd.sum_sq_err;
  c.dropped_dead = hd.dropped_dead; c.dropped_unseen = hd.dropped_unseen;
  hipError_t er = P.open();
  // plain allocations, as compact_build's (a snapshot that replaces another takes its memory right after a range of that size went back)
  if (er == hipSuccess && hd.pruned) er = fmx_dev_alloc_plain(&c.dir, (size_t)nwords * sizeof(uint2));
  if (er == hipSuccess && i8) { c.P = hd.P; er = fmx_dev_alloc_plain(&c.B, arows * hd.P); }
  if (er == hipSuccess && !i8) er = fmx_dev_alloc_plain(&c.V, arows * rs * sizeof(uint16_t));
  if (er == hipSuccess && !i8) er = fmx_dev_alloc_plain(&c.w, arows * sizeof(float));
  if (er == hipSuccess) er = fmx_dev_alloc(&c.w0, sizeof(double));
  // bf16: the padding of a row is +0 and stays so (k_snap_rows writes columns < num_factor only); the spare row of an empty table is +0 too
  if (er == hipSuccess && !i8) er = hipMemsetAsync(c.V, 0, arows * rs * sizeof(uint16_t), h->stream);
  if (er == hipSuccess && !i8 && rows == 0) er = hipMemsetAsync(c.w, 0, sizeof(float), h->stream);
  if (er == hipSuccess && i8 && rows == 0) er = hipMemsetAsync(c.B, 0, hd.P, h->stream);
  if (er != hipSuccess) return out(fail(h, FMX_E_HIP, "%s: the snapshot's tables (%llu bytes): %s", who, (unsigned long long)device_bytes(hd, rs), hipGetErrorString(er)));
  for (uint32_t si = 0; si < hd.n_sections; si++) {
    const sn::Section& s = hd.sec[si];
    const char* name = sn::section_name(s.kind);
    if (fseeko(F.f, (off_t)s.offset, SEEK_SET) != 0) return broken(FMX_E_ARG, "cannot seek", name);
    uint64_t sum = 0;
    if (s.kind == sn::SEC_W0) {
      uint8_t b[8];
      if (fread(b, 1, 8, F.f) != 8) return broken(FMX_E_ARG, "read error", name);
      sum = sn::checksum(b, 8);
      const double w0 = sn::get_f64(b);
      if (hipMemcpy(c.w0, &w0, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return broken(FMX_E_HIP, "device copy failed", name);
    } else {
      const int rc = stream_section<false>(h, who, P, F.f, c, rs, s.kind, hd, &sum);
      if (rc) return broken(rc, "stream error", name);
    }
    if (sum != s.checksum) return broken(FMX_E_ARG, "checksum mismatch", name);
    if (s.kind == sn::SEC_DIR) {
      // the directory decides where every scoring kernel reads: it is validated here, on the device, before anything can score through it
      uint32_t bad = 0;
      int rc = sum_reset(h, who, P);
      if (rc == FMX_OK) {
        hipLaunchKernelGGL(k_snap_dir_check, dim3(stream_grid(nwords)), dim3(256), 0, h->stream, (const uint2*)c.dir, nwords, n, hd.kept,
                           reinterpret_cast<uint32_t*>(P.d_sum + 1));
        if (hipGetLastError() != hipSuccess) rc = fail(h, FMX_E_HIP, "%s: the directory check could not be launched", who);
      }
      if (rc == FMX_OK) rc = sum_read(h, who, P, &sum, &bad);
      if (rc) return broken(rc, "stream error", name);
      if (bad) return broken(FMX_E_ARG, "a rank directory that is not consistent with num_attribute and kept (bases that are not the running popcounts, "
                                        "a bit beyond num_attribute, or a total other than kept)", name);
    }
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) return out(fail(h, FMX_E_HIP, "%s: the stream could not be drained", who));
  compact_release(h->compact);
  h->compact = c;
  c = CompactState();                                              // (the tables are the handle's now)
  fill_info(info, hd, file_len, device_bytes(hd, rs), since(t0), P.device_seconds);
  return FMX_OK;
}

}  // namespace

extern "C" {

int fmx_compact_save(fmx_handle h, const char* path, fmx_snap_info* info) {
  static const char who[] = "fmx_compact_save";
  if (!h) return FMX_E_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = snap_check(h, who, path); if (rc) return rc;
  const CompactState& c = h->compact;
  if (!c.w0) return fail(h, FMX_E_STATE, "%s before fmx_compact_begin / fmx_compact_load", who);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sn::Header hd;
  hd.format = c.format;
  hd.num_attribute = h->cfg.num_attribute; hd.num_factor = (uint32_t)h->cfg.num_factor;
  hd.k0 = h->cfg.k0 ? 1u : 0u; hd.k1 = h->cfg.k1 ? 1u : 0u; hd.task = (uint32_t)h->cfg.task;
  hd.min_target = h->cfg.min_target; hd.max_target = h->cfg.max_target;
  hd.pruned = c.dir ? 1u : 0u; hd.P = c.format == FMX_COMPACT_INT8 ? c.P : 0u;
  hd.kept = c.dir ? c.kept : 0;
  hd.nonfinite = c.nonfinite; hd.max_abs_err = c.max_abs_err; hd.sum_sq_err = c.sum_sq_err;
  hd.dropped_dead = c.dropped_dead; hd.dropped_unseen = c.dropped_unseen;
  const uint64_t total = sn::plan(&hd);

  Pipe P;
  CK_HIP(P.open());
  File F;
  const std::string tmp_path = std::string(path) + ".tmp";
  F.f = fopen(tmp_path.c_str(), "wb");
  if (!F.f) return fail(h, FMX_E_ARG, "%s: cannot create %s (%s)", who, tmp_path.c_str(), strerror(errno));
  F.remove_path = tmp_path;
  uint8_t head[sn::HEADER_BYTES];
  memset(head, 0, sizeof(head));                                 // (the header is written again, with the checksums, at the end)
  if (fwrite(head, 1, sizeof(head), F.f) != sizeof(head)) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
  for (uint32_t si = 0; si < hd.n_sections; si++) {
    sn::Section& s = hd.sec[si];
    if (s.kind == sn::SEC_W0) {
      uint8_t b[8];
      double w0 = 0.0;
      CK_HIP(hipMemcpy(&w0, c.w0, sizeof(double), hipMemcpyDeviceToHost));
      sn::put_f64(b, w0);
      s.checksum = sn::checksum(b, 8);
      if (fwrite(b, 1, 8, F.f) != 8) return fail(h, FMX_E_ARG, "%s: write error (%s)", who, strerror(errno));
    } else {
      rc = stream_section<true>(h, who, P, F.f, c, h->tb.rs, s.kind, hd, &s.checksum); if (rc) return rc;
    }
  }
  if ((uint64_t)ftello(F.f) != total) return fail(h, FMX_E_ARG, "%s: wrote %lld bytes where the plan has %llu", who, (long long)ftello(F.f), (unsigned long long)total);
  sn::encode(hd, head);
  if (fseeko(F.f, 0, SEEK_SET) != 0 || fwrite(head, 1, sizeof(head), F.f) != sizeof(head) || fflush(F.f) != 0)
    return fail(h, FMX_E_ARG, "%s: write error on %s (%s)", who, tmp_path.c_str(), strerror(errno));
  const int cl = fclose(F.f);
  F.f = nullptr;
  if (cl != 0) return fail(h, FMX_E_ARG, "%s: write error on %s (%s)", who, tmp_path.c_str(), strerror(errno));
  if (rename(tmp_path.c_str(), path) != 0) return fail(h, FMX_E_ARG, "%s: cannot rename %s to %s (%s)", who, tmp_path.c_str(), path, strerror(errno));
  F.remove_path.clear();
  fill_info(info, hd, total, device_bytes(hd, h->tb.rs), since(t0), P.device_seconds);
  return FMX_OK;
}

int fmx_compact_load(fmx_handle h, const char* path, fmx_snap_info* info) {
  static const char who[] = "fmx_compact_load";
  if (!h) return FMX_E_ARG;
  int rc = snap_check(h, who, path); if (rc) return rc;
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) return fail(h, FMX_E_ARG, "%s: cannot open %s (%s)", who, path, strerror(errno));
  sn::Header hd;
  uint64_t file_len = 0;
  char err[256] = "";
  if (!read_header(F.f, &hd, &file_len, err, sizeof(err))) return fail(h, FMX_E_ARG, "%s: %s: %s", who, path, err);
  return load_into(h, who, path, F, hd, file_len, info);
}

int fmx_snapshot_info(const char* path, fmx_snap_info* info, char* err, size_t err_len) {
  char local[256] = "";
  auto say = [&](const char* text) { if (err && err_len) snprintf(err, err_len, "%s", text); return FMX_E_ARG; };
  if (!path || !info) return say("fmx_snapshot_info: path or info is NULL");
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) { snprintf(local, sizeof(local), "cannot open %s (%s)", path, strerror(errno)); return say(local); }
  sn::Header hd;
  uint64_t file_len = 0;
  if (!read_header(F.f, &hd, &file_len, local, sizeof(local))) return say(local);
  fill_info(info, hd, file_len, 0, 0.0, 0.0);
  return FMX_OK;
}

int fmx_serve_open(const char* path, int device, fmx_handle* out, fmx_snap_info* info) {
  static const char who[] = "fmx_serve_open";
  if (!out) return fail(nullptr, FMX_E_ARG, "%s: out is NULL", who);
  *out = nullptr;
  if (!path) return fail(nullptr, FMX_E_ARG, "%s: path is NULL", who);
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) return fail(nullptr, FMX_E_ARG, "%s: cannot open %s (%s)", who, path, strerror(errno));
  sn::Header hd;
  uint64_t file_len = 0;
  char err[256] = "";
  if (!read_header(F.f, &hd, &file_len, err, sizeof(err))) return fail(nullptr, FMX_E_ARG, "%s: %s: %s", who, path, err);
  fmx_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.num_attribute = hd.num_attribute; cfg.num_factor = (int32_t)hd.num_factor; cfg.k0 = (int32_t)hd.k0; cfg.k1 = (int32_t)hd.k1;
  cfg.task = (int32_t)hd.task; cfg.min_target = hd.min_target; cfg.max_target = hd.max_target;
  cfg.device = device; cfg.shard_rank = 0; cfg.shard_world = 1;
  fmx_handle h = nullptr;
  int rc = create_handle(&cfg, &h, true);
  if (rc) return rc;                                               // (the reason is the creation error already)
  rc = load_into(h, who, path, F, hd, file_len, info);
  if (rc) {
    fail(nullptr, rc, "%s", h->err.c_str());
    fmx_destroy(h);
    return rc;
  }
  *out = h;
  return FMX_OK;
}

}  // extern "C"
