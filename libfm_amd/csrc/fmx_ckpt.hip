// fmx_ckpt.hip -- C-ABI (include/fmx.h "fmx_checkpoint_*"): exact binary checkpoints of the model and of an open AdaGrad / FTRL
// session.  The byte layout and everything a load refuses from the header alone is fmx_ckpt_format.h (host
// only); the kernels are fmx_ckpt_kernels.h; the two-buffer pipe a section is streamed through, and the checksum formed on the device
// by the kernel that moves it, are fmx_pipe.h (shared with fmx_snap.hip).
#include "fmx_pipe.h"
#include "fmx_ckpt_kernels.h"
#include "fmx_ckpt_format.h"

namespace {

namespace ck = fmx_ckpt;

struct DevBufs {                             // the sparse path's arrays, freed on every path out of a call
  uint32_t* flag = nullptr; uint32_t* pos = nullptr; uint32_t* ids = nullptr; void* tmp = nullptr;
  ~DevBufs() { fmx_dev_free(flag); fmx_dev_free(pos); fmx_dev_free(ids); fmx_dev_free(tmp); }
};

// rows of a chunk: as many as fit, an even number so that every chunk but the last ends on a word boundary
inline uint64_t chunk_rows(uint32_t cols) { return std::max<uint64_t>(2, (CKPT_CHUNK / ((size_t)cols * 4)) & ~size_t(1)); }

// one section of table rows, device -> file (fmx_pipe.h pipe_save around k_ckpt_rows).  *sum_out = its checksum.
int save_rows(fmx_handle h, const char* who, Pipe& P, FILE* f, const CkptRows& t, uint64_t n_rows, uint64_t* sum_out) {
  *sum_out = 0;
  if (n_rows == 0 || t.cols == 0) return FMX_OK;
  return pipe_save(h, who, P, f, n_rows, chunk_rows(t.cols), (uint64_t)t.cols * 4, [&](int b, uint64_t r0, uint64_t rows, uint64_t word0, uint32_t n_words) {
    hipLaunchKernelGGL(k_ckpt_rows<true>, dim3(stream_grid(n_words)), dim3(256), 0, h->stream, t, r0, (uint32_t)(rows * t.cols), word0, P.dev[b], P.d_sum);
  }, sum_out);
}

// one section of table rows, file -> device; with ids the rows are scattered (the list has been validated).  *sum_out = the checksum
// of what arrived in the staging buffers.
int load_rows(fmx_handle h, const char* who, Pipe& P, FILE* f, const CkptRows& t, uint64_t n_rows, uint64_t* sum_out) {
  *sum_out = 0;
  if (n_rows == 0 || t.cols == 0) return FMX_OK;
  return pipe_load(h, who, P, f, n_rows, chunk_rows(t.cols), (uint64_t)t.cols * 4, [&](int b, uint64_t r0, uint64_t rows, uint64_t word0, uint32_t n_words) {
    hipLaunchKernelGGL(k_ckpt_rows<false>, dim3(stream_grid(n_words)), dim3(256), 0, h->stream, t, r0, (uint32_t)(rows * t.cols), word0, P.dev[b], P.d_sum);
  }, sum_out);
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

uint32_t open_session(fmx_handle h) { return h->adapt.nv ? ck::SESSION_ADAGRAD : h->ftrl.nv ? ck::SESSION_FTRL : ck::SESSION_NONE; }

// what both entry points refuse from their arguments and the handle's kind
int ckpt_check(fmx_handle h, const char* who, const char* path, const fmx_ckpt_opts* opts, uint32_t* flags) {
  if (!path) return fail(h, FMX_E_ARG, "%s: path is NULL", who);
  *flags = opts ? opts->flags : 0u;
  if (*flags & ~ck::KNOWN_FLAGS) return fail(h, FMX_E_ARG, "%s: unknown flags 0x%x", who, *flags);
  if (h->cfg.shard_world > 1 || h->comm || (h->group && !h->owns_group))
    return fail(h, FMX_E_UNSUPPORTED, "%s: not supported on feature shards / communicator ranks", who);
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

}  // namespace

extern "C" {

int fmx_checkpoint_save(fmx_handle h, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_checkpoint_save";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_checkpoint_save"); if (_sr) return _sr; }
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t flags = 0;
  int rc = ckpt_check(h, who, path, opts, &flags); if (rc) return rc;
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  const uint32_t rs = h->tb.rs;

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
  // the sparse path first, so that the plan of the file is complete before its first byte: flags, their exclusive scan, the ids
  if (hd.session != ck::SESSION_NONE && dense) hd.state_rows = n;
  if (hd.session != ck::SESSION_NONE && !dense) {
    // (hipcub's item count is an int)
    if (n > 0x7FFFFFFFull) return fail(h, FMX_E_UNSUPPORTED, "%s: the sparse state of more than 2^31 - 1 features (use FMX_CKPT_DENSE_STATE)", who);
    CK_HIP(fmx_dev_alloc(&D.flag, n * 4));
    CK_HIP(fmx_dev_alloc(&D.pos, n * 4));
    CK_HIP(hipEventRecord(P.start[0], h->stream));
    const uint32_t L = (uint32_t)std::min(h->KP, 64);            // lanes per feature: a power of two
    const uint64_t waves = (n + 64 / L - 1) / (64 / L);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((waves + 3) / 4, 8192);
    if (hd.session == ck::SESSION_ADAGRAD)
      hipLaunchKernelGGL(k_ckpt_flag_adagrad, dim3(grid), dim3(256), 0, h->stream, (const float*)h->adapt.nw, (const float*)h->adapt.nv, rs, n, k, L,
                         h->adapt.init_acc, D.flag);
    else
      hipLaunchKernelGGL(k_ckpt_flag_ftrl, dim3(grid), dim3(256), 0, h->stream, h->tb, (const float*)h->ftrl.zw, (const float*)h->ftrl.zv,
                         (const float*)h->ftrl.nw, (const float*)h->ftrl.nv, n, k, L, h->ftrl.start_D(h->ftrl.l2_w), h->ftrl.l1_w,
                         h->ftrl.start_D(h->ftrl.l2_v), h->ftrl.l1_v, h->ftrl.init_acc, D.flag);
    CK_HIP(hipGetLastError());
    size_t tmp_bytes = 0;
    CK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, D.flag, D.pos, (int)n, h->stream));
    CK_HIP(fmx_dev_alloc_bytes(&D.tmp, std::max<size_t>(tmp_bytes, 8)));
    CK_HIP(hipcub::DeviceScan::ExclusiveSum(D.tmp, tmp_bytes, D.flag, D.pos, (int)n, h->stream));
    uint32_t last[2] = {0, 0};
    CK_HIP(hipMemcpyAsync(&last[0], D.pos + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(&last[1], D.flag + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    hd.state_rows = (uint64_t)last[0] + last[1];
    CK_HIP(fmx_dev_alloc(&D.ids, std::max<uint64_t>(ck::padded(hd.state_rows * 4), 8)));
    CK_HIP(hipMemsetAsync(D.ids, 0, std::max<uint64_t>(ck::padded(hd.state_rows * 4), 8), h->stream));
    hipLaunchKernelGGL(k_ckpt_compact, dim3(stream_grid(n)), dim3(256), 0, h->stream, (const uint32_t*)D.flag, (const uint32_t*)D.pos, n, D.ids);
    CK_HIP(hipGetLastError());
    CK_HIP(hipEventRecord(P.end[0], h->stream));
    P.pending[0] = true;
    CK_HIP(P.finish(0));
  }
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
    if (s.kind == ck::SEC_W0) {
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
    } else {
      CkptRows t = {nullptr, nullptr, rs, 1u, 0u, nullptr};
      uint64_t rows = n;
      if (s.kind == ck::SEC_W) { t.lin = h->tb.w; t.ls = h->tb.ws; t.cols = 1; }
      else if (s.kind == ck::SEC_V) { t.tab = h->tb.V; t.cols = (uint32_t)k; }
      else {
        const bool z = s.kind == ck::SEC_Z;
        t.tab = z ? h->ftrl.zv : hd.session == ck::SESSION_FTRL ? h->ftrl.nv : h->adapt.nv;
        t.lin = z ? h->ftrl.zw : hd.session == ck::SESSION_FTRL ? h->ftrl.nw : h->adapt.nw;
        t.cols = (uint32_t)k + 1u; t.ids = dense ? nullptr : D.ids; rows = hd.state_rows;
      }
      rc = save_rows(h, who, P, F.f, t, rows, &s.checksum); if (rc) return rc;
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

int fmx_checkpoint_load(fmx_handle h, const char* path, const fmx_ckpt_opts* opts, fmx_ckpt_info* info) {
  static const char who[] = "fmx_checkpoint_load";
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_checkpoint_load"); if (_sr) return _sr; }
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t flags = 0;
  int rc = ckpt_check(h, who, path, opts, &flags); if (rc) return rc;
  if (h->sgda.reg) return fail(h, FMX_E_STATE, "%s: an SGDA session is open (call fmx_sgda_end first)", who);
  if (h->als.slot >= 0) return fail(h, FMX_E_STATE, "%s: an ALS / MCMC session is open (call fmx_als_end first)", who);
  File F;
  F.f = fopen(path, "rb");
  if (!F.f) return fail(h, FMX_E_ARG, "%s: cannot open %s (%s)", who, path, strerror(errno));
  ck::Header hd;
  uint64_t file_len = 0;
  char err[256] = "";
  if (!read_header(F.f, &hd, &file_len, err, sizeof(err))) return fail(h, FMX_E_ARG, "%s: %s: %s", who, path, err);
  const uint64_t n = h->cfg.num_attribute;
  const int k = h->cfg.num_factor;
  if (hd.num_attribute != n) return fail(h, FMX_E_ARG, "%s: num_attribute is %llu in the file and %llu on the handle", who, (unsigned long long)hd.num_attribute, (unsigned long long)n);
  if (hd.num_factor != (uint32_t)k) return fail(h, FMX_E_ARG, "%s: num_factor is %u in the file and %d on the handle", who, hd.num_factor, k);
  if (hd.k0 != (h->cfg.k0 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k0 is %u in the file and %d on the handle", who, hd.k0, h->cfg.k0 ? 1 : 0);
  if (hd.k1 != (h->cfg.k1 ? 1u : 0u)) return fail(h, FMX_E_ARG, "%s: k1 is %u in the file and %d on the handle", who, hd.k1, h->cfg.k1 ? 1 : 0);
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
  touch_w(h);
  { int _rc = lag_flush(h); if (_rc) return _rc; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  Pipe P;
  DevBufs D;
  CK_HIP(P.open());
  auto broken = [&](int code, const char* what, const char* section) {
    const std::string before = code == FMX_E_ARG ? std::string() : h->err;    // (a HIP or read error keeps its own text in front)
    if (h->stream) hipStreamSynchronize(h->stream);
    adapt_free(h); ftrl_free(h);
    return fail(h, code, "%s: %s%s%s in section '%s' of %s: the parameters are unspecified and any AdaGrad / FTRL session has been closed",
                who, before.c_str(), before.empty() ? "" : "; ", what, section, path);
  };
  const uint32_t rs = h->tb.rs;
  bool session_ready = false;
  for (uint32_t si = 0; si < hd.n_sections; si++) {
    const ck::Section& s = hd.sec[si];
    const char* name = ck::section_name(s.kind);
    if (s.kind >= ck::SEC_IDS && !take_session) break;           // (the rest of the file is the session)
    if (s.kind >= ck::SEC_IDS && !session_ready) {
      session_ready = true;
      // the first section of the session: the parameters are in place, so its tables and their start state come first
      if (hd.session == ck::SESSION_ADAGRAD) {
        if (h->ftrl.nv) ftrl_free(h);
        rc = adapt_tables(h, who); if (rc) return broken(rc, "no memory for the session", name);
        h->adapt.eta = as.eta; h->adapt.init_acc = as.init_acc;
        rc = adapt_start_state(h);
      } else {
        if (h->adapt.nv) adapt_free(h);
        rc = ftrl_tables(h, who); if (rc) return broken(rc, "no memory for the session", name);
        fs.zw = h->ftrl.zw; fs.zv = h->ftrl.zv; fs.nw = h->ftrl.nw; fs.nv = h->ftrl.nv;
        h->ftrl = fs;
        rc = ftrl_start_state(h);
      }
      if (rc) return broken(rc, "the start state failed", name);
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
        if (hipMemcpy(h->w0, &w0, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return broken(FMX_E_HIP, "device copy failed", name);
      }
    } else if (s.kind == ck::SEC_IDS) {
      if (fmx_dev_alloc(&D.ids, std::max<uint64_t>(ck::padded(hd.state_rows * 4), 8)) != hipSuccess) return broken(FMX_E_HIP, "no memory for the id list", name);
      rc = copy_ids(h, who, P, F.f, D.ids, hd.state_rows, false); if (rc) return broken(rc, "stream error", name);
      uint32_t bad = 0;
      rc = check_ids(h, who, P, D.ids, hd.state_rows, &sum, &bad); if (rc) return broken(rc, "stream error", name);
      if (bad) return broken(FMX_E_ARG, "ids that are not strictly ascending or not below num_attribute", name);
    } else {
      CkptRows t = {nullptr, nullptr, rs, 1u, 0u, nullptr};
      uint64_t rows = n;
      if (s.kind == ck::SEC_W) { t.lin = h->tb.w; t.ls = h->tb.ws; t.cols = 1; }
      else if (s.kind == ck::SEC_V) { t.tab = h->tb.V; t.cols = (uint32_t)k; }
      else {
        const bool z = s.kind == ck::SEC_Z;
        t.tab = z ? h->ftrl.zv : hd.session == ck::SESSION_FTRL ? h->ftrl.nv : h->adapt.nv;
        t.lin = z ? h->ftrl.zw : hd.session == ck::SESSION_FTRL ? h->ftrl.nw : h->adapt.nw;
        t.cols = (uint32_t)k + 1u; t.ids = D.ids; rows = hd.state_rows;       // (D.ids is null for a dense file)
      }
      rc = load_rows(h, who, P, F.f, t, rows, &sum); if (rc) return broken(rc, "stream error", name);
    }
    if (sum != s.checksum) return broken(FMX_E_ARG, "checksum mismatch", name);
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  fill_info(info, hd, file_len, since(t0), P.device_seconds);
  return FMX_OK;
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
