// fmx_als.hip -- C-ABI (include/fmx.h): the ALS / MCMC learner (level-scheduled coordinate sweeps, fmx_als_kernels.h).
#define FMX_GRID_OVER_DEFAULT 2                    // = FMX_GRID_OVER_ALS (fmx_internal.h): the column kernels keep grid-stride workgroups
#include "fmx_internal.h"
#include "fmx_als_levels.h"

extern "C" {

// ---------------------------------------------------------------------------------------------
// ALS / MCMC
// ---------------------------------------------------------------------------------------------
extern "C++" void als_free(fmx_handle h) {
  AlsState& a = h->als;
  fmx_dev_free(a.e); fmx_dev_free(a.q); fmx_dev_free(a.seen); fmx_dev_free(a.level_list); fmx_dev_free(a.ldesc);
  fmx_dev_free(a.prior); fmx_dev_free(a.vt); fmx_dev_free(a.delta); fmx_dev_free(a.epart);
  fmx_dev_free(a.r_row); fmx_dev_free(a.r_pos); fmx_dev_free(a.r_x); fmx_dev_free(a.t_row); fmx_dev_free(a.dth);
  for (AlsBlock& b : a.blk) {
    fmx_dev_free(b.level_list); fmx_dev_free(b.cache); fmx_dev_free(b.qb_all); fmx_dev_free(b.cpart); fmx_dev_free(b.delta);
  }
  a = AlsState();
}

int fmx_als_end(fmx_handle h) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_als_end"); if (_sr) return _sr; }
  touch_w(h);
  if (!h) return FMX_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  als_free(h);
  return FMX_OK;
}

static int als_eterms(fmx_handle h, const Slot& s, EQ* e, double* q, double* e_part = nullptr) {
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_als_eterms<KP>), ((uint64_t)s.n_rows + EtermsRows<KP>::R - 1) / EtermsRows<KP>::R, h->stream, s.ent, s.row_ptr, s.n_rows, h->tb,
                                     h->cfg.k0, h->cfg.k1, h->w0, e, q, e_part));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// the rows whose columns a level build orders: the session's main rows (r < 0) or kept block r's own rows
static const Slot& als_rows(fmx_handle x, int r) {
  const Slot& s = x->slots[x->als.slot];
  return r < 0 ? s : s.blocks[r]->rows;
}

struct SegLevels { std::vector<uint32_t> rel, level; };   // a member's segments: first entry [nseg + 1] and level [nseg]

// The dependency LEVELS of one set of rows (r as in als_rows; their X^T is built, ensure_segments) over the union of the members'
// columns in GLOBAL feature order (assign_levels; host, O(nnz)).  Every member gets the same number of levels (on a shard some may be
// empty): its level_ptr and the level-ordered list of its columns on its device; seen[i] marks its columns at id offset + feature
// -- the block's attr_offset, which is 0 on a shard (its block attributes are local table rows) like the main rows'.
// segs[i]: what the split step needs of member i's segments.  *bad: the member that failed.
static int build_levels(const std::vector<fmx_handle>& hs, int r, std::vector<std::vector<uint8_t>>& seen, std::vector<SegLevels>& segs,
                        size_t* bad) {
  const size_t P = hs.size();
  std::vector<LevelCols<TEntry>> parts;
  std::vector<std::vector<uint32_t>> seg_feat(P), gid(P);
  std::vector<std::vector<TEntry>> tent(P);
  segs.assign(P, SegLevels());
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    const Slot& s = als_rows(x, r);
    const uint32_t nseg = s.nseg;
    std::vector<uint32_t>& rel = segs[i].rel;
    *bad = i;
    seg_feat[i].resize(nseg); rel.resize((size_t)nseg + 1); segs[i].level.resize(nseg); tent[i].resize((size_t)s.nnz);
    if (nseg) {
      HIPCHK(x, hipSetDevice(x->device));
      HIPCHK(x, hipMemcpy(seg_feat[i].data(), s.seg_feat, (size_t)nseg * 4, hipMemcpyDeviceToHost));
      HIPCHK(x, hipMemcpy(rel.data(), s.seg_rel, (size_t)nseg * 4, hipMemcpyDeviceToHost));
      HIPCHK(x, hipMemcpy(tent[i].data(), s.t_ent, (size_t)s.nnz * sizeof(TEntry), hipMemcpyDeviceToHost));
    }
    rel[nseg] = (uint32_t)s.nnz;
    const Shard sh = make_shard(x->cfg);
    if (sh.world > 1) {                                              // (unsharded: the table row is the global id)
      gid[i].resize(nseg);
      for (uint32_t sg = 0; sg < nseg; sg++) gid[i][sg] = sh.global(seg_feat[i][sg]);
    }
    parts.push_back({nseg, sh.world > 1 ? gid[i].data() : seg_feat[i].data(), rel.data(), tent[i].data(), segs[i].level.data()});
  }
  const uint32_t n_levels = assign_levels(parts, als_rows(hs[0], r).n_rows);
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    AlsState& a = x->als;
    const uint32_t nseg = als_rows(x, r).nseg;
    const uint32_t id_offset = r < 0 ? 0u : x->slots[a.slot].blocks[r]->attr_offset;
    const std::vector<uint32_t>& lvl = segs[i].level;
    std::vector<uint32_t>& lp = r < 0 ? a.level_ptr : a.blk[r].level_ptr;
    uint32_t** d_list = r < 0 ? &a.level_list : &a.blk[r].level_list;
    *bad = i;
    lp.assign((size_t)n_levels + 1, 0);
    for (uint32_t sg = 0; sg < nseg; sg++) lp[lvl[sg] + 1]++;
    for (uint32_t l = 0; l < n_levels; l++) lp[l + 1] += lp[l];
    std::vector<uint32_t> list(std::max<uint32_t>(nseg, 1)), fill(lp.begin(), lp.end());
    for (uint32_t sg = 0; sg < nseg; sg++) list[fill[lvl[sg]]++] = sg;
    for (uint32_t sg = 0; sg < nseg; sg++) seen[i][(size_t)id_offset + seg_feat[i][sg]] = 1;
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, fmx_dev_alloc(d_list, list.size() * 4));
    HIPCHK(x, hipMemcpy(*d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice));
  }
  *bad = 0;
  return FMX_OK;
}

// the split step's view of one member's levels: where every segment sits inside its level's list (seg_pos) and the entry range of
// every level (AlsState::lev_ent)
static void level_entries(const SegLevels& sl, AlsState& a, std::vector<uint32_t>& seg_pos) {
  const size_t nseg = sl.level.size(), n_levels = a.level_ptr.size() - 1;
  std::vector<uint32_t> fill(n_levels, 0);
  seg_pos.assign(std::max<size_t>(nseg, 1), 0);
  a.lev_ent.assign(n_levels + 1, 0);
  for (size_t sg = 0; sg < nseg; sg++) {
    seg_pos[sg] = fill[sl.level[sg]]++;
    a.lev_ent[sl.level[sg] + 1] += sl.rel[sg + 1] - sl.rel[sg];
  }
  for (size_t l = 0; l < n_levels; l++) a.lev_ent[l + 1] += a.lev_ent[l];
}

// a kept block's rows: their partial sums (lin - 0.5 * sum of squares -> cpart, factor sums -> qb_all), each block row once
static int block_eterms(fmx_handle h, const BlockRows& br, AlsBlock& ab) {
  const uint32_t B = br.rows.n_rows;
  Tab tb = h->tb;                                            // the block's attribute 0 is global attribute attr_offset (a shard: local rows, offset 0)
  tb.V += (size_t)br.attr_offset * tb.rs; tb.w += (size_t)br.attr_offset * tb.ws;
  KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_als_eterms<KP>), ((uint64_t)B + EtermsRows<KP>::R - 1) / EtermsRows<KP>::R, h->stream, br.rows.ent, br.rows.row_ptr, B, tb,
                                     0, h->cfg.k1, (const double*)h->w0, (EQ*)nullptr, ab.qb_all, ab.cpart));
  HIPCHK(h, hipGetLastError());
  return FMX_OK;
}

// y-hat (and q_f for the coming sweep) of the session's rows, on every member.  The main rows and every kept block's rows are
// summed separately -- a block row once, however many main rows map to it -- over the member's own features; feature shards (g)
// all-reduce these partial sums; then every member adds the blocks' sums to the main rows' through the mappings -- identically, so
// each block counts once -- and squares the COMPLETE factor sums (k_als_set_e).  One member without blocks has nothing to add:
// k_als_eterms finishes e itself (no pass over epart, and e keeps that kernel's order of sums).  *bad: the member that failed.
static int als_repredict(const std::vector<fmx_handle>& hs, fmx_group g /* nullptr: nothing is exchanged */, size_t* bad) {
  const size_t P = hs.size();
  fmx_handle h0 = hs[0];
  const Slot& s0 = h0->slots[h0->als.slot];
  const uint32_t N = s0.n_rows;
  const int kf = h0->cfg.num_factor;
  const size_t R = s0.blocks.size();
  const bool direct = !g && R == 0;
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    AlsState& a = x->als;
    const Slot& s = x->slots[a.slot];
    *bad = i;
    HIPCHK(x, hipSetDevice(x->device));
    int rc = als_eterms(x, s, a.e, a.q, direct ? nullptr : a.epart);
    for (size_t r = 0; r < R && rc == FMX_OK; r++) rc = block_eterms(x, *s.blocks[r], a.blk[r]);
    if (rc) return rc;
  }
  *bad = 0;
  if (direct) return FMX_OK;
  if (g) {
    std::vector<double*> bq(P), be(P);
    for (size_t i = 0; i < P; i++) { bq[i] = hs[i]->als.q; be[i] = hs[i]->als.epart; }
    int rc = kf > 0 ? group_allreduce_f64(g, bq, (size_t)kf * N) : FMX_OK;      // q is [KP][N]: the first k factor rows
    if (rc == FMX_OK) rc = group_allreduce_f64(g, be, N);
    for (size_t r = 0; r < R && rc == FMX_OK; r++) {
      const uint32_t B = s0.blocks[r]->rows.n_rows;
      for (size_t i = 0; i < P; i++) { bq[i] = hs[i]->als.blk[r].qb_all; be[i] = hs[i]->als.blk[r].cpart; }
      rc = kf > 0 ? group_allreduce_f64(g, bq, (size_t)kf * B) : FMX_OK;        // qb_all is [KP][B]
      if (rc == FMX_OK) rc = group_allreduce_f64(g, be, B);
    }
    if (rc) return rc;
  }
  const dim3 g1(std::min<uint32_t>((N + 255) / 256, 2048)), b1(256);
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    AlsState& a = x->als;
    const Slot& s = x->slots[a.slot];
    *bad = i;
    HIPCHK(x, hipSetDevice(x->device));
    for (size_t r = 0; r < R; r++)
      hipLaunchKernelGGL(k_rel_combine, g1, b1, 0, x->stream, s.blocks[r]->map, N, s.blocks[r]->rows.n_rows, a.blk[r].cpart, a.blk[r].qb_all,
                         kf, a.epart, a.q);
    hipLaunchKernelGGL(k_als_set_e, g1, b1, 0, x->stream, a.e, a.epart, a.q, kf, N, x->cfg.k0, x->w0);
    HIPCHK(x, hipGetLastError());
  }
  *bad = 0;
  return FMX_OK;
}

// the split step's row-ordered copy of X^T (AlsState::r_*): device radix sort of the entries by (level of the feature, row)
static int als_build_rows(fmx_handle h, const Slot& s, AlsState& a, const std::vector<uint32_t>& seg_level, const std::vector<uint32_t>& seg_pos) {
  const uint32_t nnz = (uint32_t)s.nnz, nseg = s.nseg;
  hipStream_t st = h->stream;
  uint64_t *ka = nullptr, *kb = nullptr; uint32_t *va = nullptr, *vb = nullptr, *d_lvl = nullptr, *d_pos = nullptr; void* tmp = nullptr;
  int rc = FMX_OK;
#define ROW_CHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    rc = fail(h, FMX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); goto done; } } while (0)
  {
    uint32_t big = 1;
    for (size_t l = 0; l + 1 < a.level_ptr.size(); l++) big = std::max(big, a.level_ptr[l + 1] - a.level_ptr[l]);
    int bits_level = 1; while ((1ull << bits_level) < a.level_ptr.size()) bits_level++;
    size_t tmp_bytes = 0;
    const dim3 gr(std::min<uint32_t>((nnz + 255) / 256, 8192)), bl(256);
    ROW_CHK(fmx_dev_alloc(&ka, (size_t)nnz * 8)); ROW_CHK(fmx_dev_alloc(&kb, (size_t)nnz * 8));
    ROW_CHK(fmx_dev_alloc(&va, (size_t)nnz * 4)); ROW_CHK(fmx_dev_alloc(&vb, (size_t)nnz * 4));
    ROW_CHK(fmx_dev_alloc(&d_lvl, (size_t)nseg * 4)); ROW_CHK(fmx_dev_alloc(&d_pos, (size_t)nseg * 4));
    ROW_CHK(fmx_dev_alloc(&a.r_row, (size_t)nnz * 4)); ROW_CHK(fmx_dev_alloc(&a.r_pos, (size_t)nnz * 4)); ROW_CHK(fmx_dev_alloc(&a.r_x, (size_t)nnz * 4));
    ROW_CHK(fmx_dev_alloc(&a.dth, (size_t)big * sizeof(float2)));
    ROW_CHK(hipMemcpyAsync(d_lvl, seg_level.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, st));
    ROW_CHK(hipMemcpyAsync(d_pos, seg_pos.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_als_rowkeys, gr, bl, 0, st, s.t_ent, s.seg_rel, nseg, nnz, d_lvl, ka, va);
    ROW_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ka, kb, va, vb, (int)nnz, 0, 32 + bits_level, st));
    ROW_CHK(fmx_dev_alloc(&tmp, tmp_bytes));
    ROW_CHK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, ka, kb, va, vb, (int)nnz, 0, 32 + bits_level, st));
    hipLaunchKernelGGL(k_als_rowfill, gr, bl, 0, st, s.t_ent, s.seg_rel, nseg, nnz, d_pos, vb, a.r_row, a.r_pos, a.r_x);
    ROW_CHK(hipGetLastError());
    {  // which levels hold every row exactly once, in order (one-hot fields)
      const size_t nl = a.lev_ent.size() - 1;
      a.lev_dense.assign(nl, 0);
      std::vector<uint32_t> flags(nl, 1u);
      ROW_CHK(hipMemsetAsync(d_lvl, 0, std::min<size_t>(nl, nseg) * 4, st));          // (d_lvl is free after the sort keys were made)
      for (size_t l = 0; l < nl && l < nseg; l++)
        if (a.lev_ent[l + 1] - a.lev_ent[l] == s.n_rows)
          hipLaunchKernelGGL(k_als_rows_check_dense, dim3(std::min<uint32_t>((s.n_rows + 255) / 256, 4096)), bl, 0, st, a.r_row + a.lev_ent[l],
                             a.r_x + a.lev_ent[l], s.n_rows, d_lvl + l);
      ROW_CHK(hipMemcpyAsync(flags.data(), d_lvl, std::min<size_t>(nl, nseg) * 4, hipMemcpyDeviceToHost, st));
      ROW_CHK(hipStreamSynchronize(st));
      bool any_unit = false;
      for (size_t l = 0; l < nl && l < nseg; l++) {
        const bool dense = a.lev_ent[l + 1] - a.lev_ent[l] == s.n_rows && (flags[l] & 1u) == 0;
        a.lev_dense[l] = dense ? ((flags[l] & 2u) ? 1 : 2) : 0;
        any_unit = any_unit || a.lev_dense[l] == 2;
      }
      if (any_unit) {                                                // the row-only stream of X^T for the levels of unit values
        ROW_CHK(fmx_dev_alloc(&a.t_row, (size_t)nnz * 4));
        hipLaunchKernelGGL(k_als_trow, gr, bl, 0, st, s.t_ent, (uint32_t)nnz, a.t_row);
        ROW_CHK(hipGetLastError());
        ROW_CHK(hipStreamSynchronize(st));
      }
    }
  }
done:
#undef ROW_CHK
  for (void* p : {(void*)ka, (void*)kb, (void*)va, (void*)vb, (void*)d_lvl, (void*)d_pos, tmp}) if (p) fmx_dev_free(p);
  return rc;
}

// lanes per column of a kept block's draws (k_rel_draw) from the mean column length
static int block_lanes(const Slot& rows) {
  const double avg_col = rows.nseg ? (double)rows.nnz / (double)rows.nseg : 0.0;
  return avg_col <= 5.0 ? 4 : (avg_col <= 12.0 ? 8 : (avg_col <= 40.0 ? 16 : 64));
}

// The set-up of a session over a list of members: one unsharded handle (g == nullptr: nothing is exchanged) or the feature shards
// of g.  Every member builds X^T of its own features -- of the main rows and of every kept block's rows; the levels are global
// (build_levels) and the first prediction is all-reduced (als_repredict).  `who`: the entry point, for the messages.  *bad: the
// member that failed; the entry points take a failed set-up's session down again.
static int als_begin_shards(const std::vector<fmx_handle>& hs, fmx_group g, int train_slot, const char* who, size_t* bad) {
  const size_t P = hs.size();
  const bool sharded = g != nullptr;
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    *bad = i;
    int rc = check_slot(x, train_slot, true);
    if (rc == FMX_OK) rc = lag_flush(x);
    if (rc) return rc;
    if (!sharded && x->cfg.shard_world > 1)
      return fail(x, FMX_E_STATE, "ALS / MCMC on a feature shard: use fmx_group_als_begin (the dependency levels are global)");
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, hipStreamSynchronize(x->stream));
    als_free(x);
    Slot& s = x->slots[train_slot];
    const Slot& s0 = hs[0]->slots[train_slot];
    if (s.n_rows == 0) return fail(x, FMX_E_ARG, "%s: empty training set", who);
    if (s.n_rows != s0.n_rows) return fail(x, FMX_E_STATE, "the shards hold different numbers of rows");
    if (s.blocks.size() != s0.blocks.size()) return fail(x, FMX_E_STATE, "the shards hold different relation blocks");
    for (size_t r = 0; r < s.blocks.size(); r++)
      if (s.blocks[r]->rows.n_rows != s0.blocks[r]->rows.n_rows) return fail(x, FMX_E_STATE, "the shards hold different relation blocks");
    rc = ensure_segments(x, s, s.n_rows);          // one "batch" = the whole data set: X^T with columns in id order
    for (size_t r = 0; r < s.blocks.size() && rc == FMX_OK; r++) {        // X^T of every block (a shard that owns none of a block's
      Slot& rows = s.blocks[r]->rows;                                     // attributes has no columns there)
      if (!sharded || rows.nnz) rc = ensure_segments(x, rows, std::max<uint32_t>(rows.n_rows, 1));
    }
    if (rc) return rc;
    x->als.slot = train_slot;
    x->als.blk.resize(s.blocks.size());
  }
  const Slot& s0 = hs[0]->slots[train_slot];
  const uint32_t N = s0.n_rows;
  const size_t R = s0.blocks.size();
  // ---- dependency levels of the main features, then -- kept `-relation` blocks -- of every block's attributes over
  //      the block's own rows (two block attributes conflict iff they share a block row)
  std::vector<std::vector<uint8_t>> seen(P);
  for (size_t i = 0; i < P; i++) seen[i].assign((size_t)hs[i]->n_local, 0);
  std::vector<SegLevels> segs;
  int rc = build_levels(hs, -1, seen, segs, bad);
  if (rc) return rc;
  if (!sharded) {
    // levels with many entries take the split step (column sums + draw, then the {e, q} update as a row-ordered stream):
    // a fused draw pays two random touches of the {e, q} cache per entry, the split one.  fmx_config::als_split_min: threshold in
    // entries per level; small levels are launch-bound and stay fused.
    fmx_handle h = hs[0];
    AlsState& a = h->als;
    a.split_min = h->cfg.als_split_min == 0 ? 65536u : (h->cfg.als_split_min == 0xFFFFFFFFu ? 0u : h->cfg.als_split_min);
    std::vector<uint32_t> seg_pos;
    level_entries(segs[0], a, seg_pos);
    bool any = false;
    for (size_t l = 0; a.split_min && l + 1 < a.lev_ent.size(); l++) any = any || (a.lev_ent[l + 1] - a.lev_ent[l] >= a.split_min);
    if (any && s0.nnz > 0 && s0.nnz < (1ull << 32)) { rc = als_build_rows(h, s0, a, segs[0].level, seg_pos); if (rc) return rc; }
    else a.split_min = 0;
  }
  for (size_t r = 0; r < R; r++) { rc = build_levels(hs, (int)r, seen, segs, bad); if (rc) return rc; }
  // ---- the session's buffers; a sharded one also records what a step's draws change (delta) and all-reduces partial sums (epart)
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    AlsState& a = x->als;
    const Slot& s = x->slots[train_slot];
    *bad = i;
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, fmx_dev_alloc(&a.seen, seen[i].size()));
    HIPCHK(x, hipMemcpy(a.seen, seen[i].data(), seen[i].size(), hipMemcpyHostToDevice));
    HIPCHK(x, fmx_dev_alloc(&a.e, (size_t)N * sizeof(EQ)));
    HIPCHK(x, fmx_dev_alloc(&a.q, (size_t)N * (size_t)x->KP * sizeof(double)));
    if (sharded) {
      HIPCHK(x, fmx_dev_alloc(&a.delta, (size_t)N * sizeof(EQ)));
      HIPCHK(x, hipMemsetAsync(a.delta, 0, (size_t)N * sizeof(EQ), x->stream));
    }
    if (sharded || R) HIPCHK(x, fmx_dev_alloc(&a.epart, (size_t)N * sizeof(double)));
    if (x->cfg.num_factor > 0 && s.nseg > 0) {
      a.vt_stride = ((size_t)s.nseg + 63) & ~(size_t)63;
      HIPCHK(x, fmx_dev_alloc(&a.vt, (size_t)x->cfg.num_factor * a.vt_stride * sizeof(float)));
    }
    for (size_t r = 0; r < R; r++) {         // the kept blocks' caches (on shards: replicated, with their per-level changes)
      const Slot& rows = s.blocks[r]->rows;
      AlsBlock& ab = a.blk[r];
      const size_t B = std::max<uint32_t>(rows.n_rows, 1);
      HIPCHK(x, fmx_dev_alloc(&ab.cache, (size_t)7 * B * sizeof(double)));
      HIPCHK(x, hipMemsetAsync(ab.cache, 0, (size_t)7 * B * sizeof(double), x->stream));
      HIPCHK(x, fmx_dev_alloc(&ab.qb_all, (size_t)x->KP * B * sizeof(double)));
      HIPCHK(x, fmx_dev_alloc(&ab.cpart, B * sizeof(double)));
      if (sharded) {
        HIPCHK(x, fmx_dev_alloc(&ab.delta, (size_t)4 * B * sizeof(double)));
        HIPCHK(x, hipMemsetAsync(ab.delta, 0, (size_t)4 * B * sizeof(double), x->stream));
      }
      ab.lanes = block_lanes(rows);
    }
  }
  // ---- first prediction and e -= target (fm_learn_mcmc_simultaneous.h:69-86)
  rc = als_repredict(hs, g, bad);
  if (rc) return rc;
  const dim3 g1(std::min<uint32_t>((N + 255) / 256, 2048)), b1(256);
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    *bad = i;
    HIPCHK(x, hipSetDevice(x->device));
    hipLaunchKernelGGL(k_als_sub_target, g1, b1, 0, x->stream, x->als.e, x->slots[train_slot].target, N);
    HIPCHK(x, hipGetLastError());
    HIPCHK(x, hipStreamSynchronize(x->stream));
  }
  *bad = 0;
  return FMX_OK;
}

int fmx_als_begin(fmx_handle h, int train_slot) {
  if (!h) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_als_begin"); if (_sr) return _sr; }
  touch_w(h);
  if (!h) return FMX_E_ARG;
  { const int rw = refuse_weighted(h, train_slot, "fmx_als_begin"); if (rw) return rw; }
  size_t bad = 0;
  const int rc = als_begin_shards(std::vector<fmx_handle>(1, h), nullptr, train_slot, "fmx_als_begin", &bad);
  if (rc != FMX_OK && h->als.slot == train_slot) als_free(h);      // a failed set-up leaves no half-built session behind
  return rc;
}

int fmx_als_moments(fmx_handle h, double* out) {
  if (!h || !out) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_als_moments"); if (_sr) return _sr; }
  AlsState& a = h->als;
  if (a.slot < 0) return fail(h, FMX_E_STATE, "fmx_als_moments before fmx_als_begin");
  HIPCHK(h, hipSetDevice(h->device));
  const Slot& s = h->slots[a.slot];
  const int k = h->cfg.num_factor;
  const uint32_t G = h->num_groups;
  const size_t cells = (size_t)(1 + h->KP) * G * 2;              // device block [1 + KP][G][2]
  double* d = nullptr;
  HIPCHK(h, fmx_dev_alloc(&d, (2 + cells) * sizeof(double)));
  hipStream_t st = h->stream;
  hipError_t er = hipMemsetAsync(d, 0, (2 + cells) * sizeof(double), st);
  const dim3 b1(256), ge(std::min<uint32_t>((s.n_rows + 255) / 256, 2048));
  hipLaunchKernelGGL(k_als_sum_e, ge, b1, 0, st, a.e, s.n_rows, d);            // d[0] = sum e, d[1] = sum e^2
  const bool grouped = G > 1;
  const int lds_ok = cells * sizeof(double) <= 64 * 1024;
  const size_t lds = (grouped && lds_ok) ? cells * sizeof(double) : 0;
  KP_SWITCH(h->KP, {
    const uint64_t waves = (h->n_local + Map<KP>::EPI - 1) / Map<KP>::EPI;
    if (grouped) { auto kf = k_group_moments<KP, true>;
      hipLaunchKernelGGL(kf, dim3(resident_grid(h, (const void*)kf, waves)), b1, lds, st, h->tb, h->n_local, h->cfg.k1, h->grp, G, lds_ok, d + 2);
    } else { auto kf = k_group_moments<KP, false>;
      hipLaunchKernelGGL(kf, dim3(resident_grid(h, (const void*)kf, waves)), b1, 0, st, h->tb, h->n_local, h->cfg.k1, h->grp, G, 0, d + 2);
    }
  });
  std::vector<double> host(2 + cells);
  if (er == hipSuccess) er = hipGetLastError();
  if (er == hipSuccess) er = hipMemcpyAsync(host.data(), d, (2 + cells) * sizeof(double), hipMemcpyDeviceToHost, st);
  if (er == hipSuccess) er = hipStreamSynchronize(st);
  fmx_dev_free(d);
  if (er != hipSuccess) return fail(h, FMX_E_HIP, "fmx_als_moments: %s", hipGetErrorString(er));
  out[0] = host[1]; out[1] = host[0];                                          // documented order: sum e^2 first
  memcpy(out + 2, host.data() + 2, (size_t)(1 + k) * G * 2 * sizeof(double)); // rows 0..k of [1 + KP][G][2]
  return FMX_OK;
}

// the draw kernels' lanes per column as a constant, in KP_SWITCH's style: inside the statement LANES is 4, 8, 16 or 64
#define LANES_SWITCH(LV, ...)                                      \
  switch (LV) {                                                    \
    case 4:  { constexpr int LANES = 4;  __VA_ARGS__; } break;     \
    case 8:  { constexpr int LANES = 8;  __VA_ARGS__; } break;     \
    case 16: { constexpr int LANES = 16; __VA_ARGS__; } break;     \
    default: { constexpr int LANES = 64; __VA_ARGS__; } break;     \
  }

// one iteration of _learn over a list of feature shards (one unsharded handle: the list has one member and nothing is
// exchanged).  Shards: the {e, q} cache is replicated; the draws of a (family, level) step record their changes
// (AlsState::delta), one all-reduce per step sums them and every shard applies the same sum -- the replicas stay identical
// bit for bit; the re-prediction all-reduces the partial y-hat and q_f of the shards ("the simple
// version").  The levels are GLOBAL (fmx_group_als_begin), so the sweep is the reference's Gauss-Seidel order whatever
// the number of shards.
static int als_sweep_shards(const std::vector<fmx_handle>& hs, fmx_group g, const fmx_als_opts* opts, fmx_als_stats* stats) {
  for (fmx_handle m : hs) touch_w(m);
  fmx_handle h = hs[0];
  const size_t P = hs.size();
  const bool sharded = g != nullptr && P > 1;
  for (fmx_handle x : hs) {
    if (x->als.slot < 0) return fail(h, FMX_E_STATE, "fmx_als_sweep before fmx_als_begin");
    if (opts->num_groups != 0 && opts->num_groups != x->num_groups)     // validated BEFORE the first device write of the sweep
      return fail(h, FMX_E_ARG, "fmx_als_sweep: opts->num_groups = %u but the handle has %u attribute groups", opts->num_groups, x->num_groups);
  }
  AlsState& a0 = h->als;
  const uint32_t N = h->slots[a0.slot].n_rows;
  const uint32_t n_levels = (uint32_t)a0.level_ptr.size() - 1;
  const dim3 g1(std::min<uint32_t>((N + 255) / 256, 2048)), b1(256);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  double acc[4] = {0, 0, 0, 0};
  // sum e, sum e^2 (draw_w0's numerator; draw_alpha's statistic for the caller): the replicas are identical, shard 0 answers
  HIPCHK(h, hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  hipLaunchKernelGGL(k_als_sum_e, g1, b1, 0, h->stream, a0.e, N, h->acc);
  HIPCHK(h, hipMemcpyAsync(acc, h->acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  double w0 = 0;
  HIPCHK(h, hipMemcpyAsync(&w0, h->w0, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stats) stats->sum_e_sqr = acc[1];
  std::mt19937_64 rng(opts->seed * 0x9E3779B97F4A7C15ull + a0.iter + 1);
  std::normal_distribution<double> nd(0.0, 1.0);
  if (h->cfg.k0) {                                         // draw_w0, fm_learn_mcmc.h:643-683 (w0_mean_0 = 0)
    double mean = acc[0] - (double)N * w0;
    const double sigma_sqr = 1.0 / (h->cfg.reg0 + opts->alpha * (double)N);
    mean = -sigma_sqr * (opts->alpha * mean - 0.0 * h->cfg.reg0);
    double nw0 = opts->do_sample ? mean + std::sqrt(sigma_sqr) * nd(rng) : mean;
    if (!(std::isnan(nw0) || std::isinf(nw0))) {
      for (fmx_handle x : hs) {
        HIPCHK(x, hipSetDevice(x->device));
        HIPCHK(x, hipMemcpyAsync(x->w0, &nw0, sizeof(double), hipMemcpyHostToDevice, x->stream));
        hipLaunchKernelGGL(k_als_add_const, g1, b1, 0, x->stream, x->als.e, N, nw0 - w0);
        HIPCHK(x, hipStreamSynchronize(x->stream));        // nw0 lives on this stack frame
      }
    }
  }
  // ---- priors per coordinate family and attribute group: [1 + k][2][NG] = lambda[NG] then mu[NG]
  const uint32_t NG = h->num_groups;
  const int kf = h->cfg.num_factor;
  const bool tabs = opts->num_groups != 0;
  std::vector<int> lanes(P);
  for (size_t i = 0; i < P; i++) {
    fmx_handle x = hs[i];
    AlsState& a = x->als;
    HIPCHK(x, hipSetDevice(x->device));
    a.prior_host.resize((size_t)(1 + kf) * 2 * NG);
    for (uint32_t gg = 0; gg < NG; gg++) {
      a.prior_host[gg] = (tabs && opts->w_lambda_g) ? opts->w_lambda_g[gg] : opts->w_lambda;
      a.prior_host[NG + gg] = (tabs && opts->w_mu_g) ? opts->w_mu_g[gg] : opts->w_mu;
      for (int f = 0; f < kf; f++) {
        double* row = a.prior_host.data() + (size_t)(1 + f) * 2 * NG;
        row[gg] = (tabs && opts->v_lambda_gf) ? opts->v_lambda_gf[(size_t)gg * kf + f] : (opts->v_lambda_f ? opts->v_lambda_f[f] : opts->v_lambda);
        row[NG + gg] = (tabs && opts->v_mu_gf) ? opts->v_mu_gf[(size_t)gg * kf + f] : (opts->v_mu_f ? opts->v_mu_f[f] : opts->v_mu);
      }
    }
    if (!a.prior) HIPCHK(x, fmx_dev_alloc(&a.prior, a.prior_host.size() * sizeof(double)));
    HIPCHK(x, hipMemcpyAsync(a.prior, a.prior_host.data(), a.prior_host.size() * sizeof(double), hipMemcpyHostToDevice, x->stream));
    // lanes per column from the mean column length (one-hot data: a handful of rows per feature)
    const Slot& s = x->slots[a.slot];
    if (!a.ldesc && s.nseg) {                                // the level-ordered column records, once per session
      HIPCHK(x, fmx_dev_alloc(&a.ldesc, (size_t)s.nseg * sizeof(uint4)));
      hipLaunchKernelGGL(k_als_ldesc, dim3(std::min<uint32_t>((s.nseg + 255) / 256, 8192)), dim3(256), 0, x->stream, a.level_list, s.nseg,
                         s.seg_feat, s.seg_rel, s.nseg, (uint32_t)s.nnz, a.ldesc);
      HIPCHK(x, hipGetLastError());
    }
    const double avg_col = s.nseg ? (double)s.nnz / (double)s.nseg : 0.0;
    // (measured at 6.7 entries per column, inside one process: 4 lanes 161.4 ms per sweep, 8 lanes 164.4, 16 lanes 195)
    lanes[i] = avg_col <= 8.0 ? 4 : (avg_col <= 16.0 ? 8 : (avg_col <= 40.0 ? 16 : 64));
  }
  // one (family, level) step on every shard, then -- shards only -- the exchange of the recorded changes
  auto level_step = [&](uint32_t l, int f /* -1: linear weights */) -> int {
    bool any = false;
    for (size_t i = 0; i < P; i++) {
      fmx_handle h = hs[i];                                  // (the launch macros refer to `h`)
      AlsState& a = h->als;
      const Slot& s = h->slots[a.slot];
      const uint32_t cnt = a.level_ptr[l + 1] - a.level_ptr[l];
      if (!cnt) continue;
      any = true;
      HIPCHK(h, hipSetDevice(h->device));
      hipStream_t st = h->stream;
      const Shard sh = make_shard(h->cfg);
      EQ* delta = sharded ? a.delta : nullptr;
      const uint32_t n_ent = (!sharded && a.split_min && a.r_row) ? a.lev_ent[l + 1] - a.lev_ent[l] : 0u;
      float2* dth = (n_ent && n_ent >= a.split_min) ? a.dth : nullptr;     // split step for this level?
      const bool unit = dth && l < a.lev_dense.size() && a.lev_dense[l] == 2 && a.t_row;   // every value of the level is 1: 4-byte streams
      const uint32_t* unit_rows = unit ? a.t_row : nullptr;
      const float* lev_x = (dth && !unit) ? a.r_x + a.lev_ent[l] : nullptr;   // (no split step: the row-ordered lists do not exist)
      // the family's parameter of a column -- v_f by its position in the level-ordered shadow where the session keeps one -- its
      // priors and its random stream
      const bool by_pos = f >= 0 && a.vt;
      float* param = f < 0 ? h->tb.w : (by_pos ? a.vt + (size_t)f * a.vt_stride : h->tb.V + f);
      const uint32_t pstride = f < 0 ? h->tb.ws : (by_pos ? 1u : h->tb.rs);
      const double* lam = f < 0 ? a.prior : a.prior + (size_t)(1 + f) * 2 * NG;
      const uint64_t stream_id = f < 0 ? mcmc_stream(a.iter, MCMC_W) : mcmc_stream(a.iter, MCMC_V, f);
      const uint32_t e0 = dth ? a.lev_ent[l] : 0u;
      const dim3 gr(std::min<uint32_t>((n_ent + 255) / 256, 16384));
#define FMX_LEVEL_STEP(ISV)                                                                                                                  \
      LANES_SWITCH(lanes[i], FMX_LAUNCH_WAVES((k_als_draw<ISV, LANES>), ((uint64_t)cnt * LANES + 63) / 64, st, s.t_ent, unit_rows,              \
                   a.ldesc + a.level_ptr[l], cnt, param, pstride, by_pos ? 1 : 0, by_pos ? a.level_ptr[l] : 0u, a.e, opts->alpha, lam, lam + NG, \
                   h->grp, opts->do_sample, opts->seed, stream_id, sh, delta, dth));                                                            \
      if (dth && a.lev_dense[l]) hipLaunchKernelGGL((k_als_rows_dense<ISV>), gr, b1, 0, st, a.r_pos + e0, lev_x, n_ent, dth, a.e);              \
      else if (dth) hipLaunchKernelGGL((k_als_rows<ISV>), gr, b1, 0, st, a.r_row + e0, a.r_pos + e0, a.r_x + e0, n_ent, dth, a.e)
      if (f < 0) { FMX_LEVEL_STEP(false); } else { FMX_LEVEL_STEP(true); }
#undef FMX_LEVEL_STEP
      HIPCHK(h, hipGetLastError());
    }
    if (sharded && any) {
      std::vector<double*> bufs(P);
      for (size_t i = 0; i < P; i++) bufs[i] = reinterpret_cast<double*>(hs[i]->als.delta);
      int rc = group_allreduce_f64(g, bufs, (size_t)N * 2);
      if (rc) return rc;
      for (fmx_handle x : hs) {
        HIPCHK(x, hipSetDevice(x->device));
        hipLaunchKernelGGL(k_als_apply_delta, g1, b1, 0, x->stream, x->als.e, x->als.delta, N);
        HIPCHK(x, hipGetLastError());
      }
    }
    return FMX_OK;
  };
  // kept `-relation` blocks: after the main features of a family, every block in turn -- caches from the main rows, the block's
  // attributes level by level on the caches, the accumulated changes back (fm_learn_mcmc.h:478-509 for w, :603-633 for v_f).
  // Shards: the caches are replicated (built from the replicated {e, q} and the all-reduced block sums); the block levels are
  // GLOBAL, each shard draws its own attributes of a level and records the cache changes (AlsBlock::delta), one all-reduce of
  // 4 B doubles per level sums them and every shard applies the sum
  auto block_steps = [&](int f /* -1: linear weights */) -> int {
    const size_t R = hs[0]->slots[a0.slot].blocks.size();
    for (size_t r = 0; r < R; r++) {
      const uint32_t B = hs[0]->slots[a0.slot].blocks[r]->rows.n_rows;
      if (!B) continue;
      const dim3 gb(std::min<uint32_t>((B + 31) / 32, 2048)), gq(std::min<uint32_t>((B + 255) / 256, 2048));
      for (fmx_handle x : hs) {
        AlsState& a = x->als;
        const BlockRows& br = *x->slots[a.slot].blocks[r];
        AlsBlock& ab = a.blk[r];
        HIPCHK(x, hipSetDevice(x->device));
        if (f >= 0) {
          hipLaunchKernelGGL(k_rel_load_qb, gq, b1, 0, x->stream, ab.cache, (const double*)(ab.qb_all + (size_t)f * B), B);
          hipLaunchKernelGGL((k_rel_aggregate<true, 8>), gb, b1, 0, x->stream, br.brow_ptr, br.brow_list, B, (const EQ*)a.e, ab.cache);
        } else {
          hipLaunchKernelGGL((k_rel_aggregate<false, 8>), gb, b1, 0, x->stream, br.brow_ptr, br.brow_list, B, (const EQ*)a.e, ab.cache);
        }
      }
      const uint64_t stream_id = f < 0 ? mcmc_stream(a0.iter, MCMC_W) : mcmc_stream(a0.iter, MCMC_V, f);
      const uint32_t nl = (uint32_t)a0.blk[r].level_ptr.size() - 1;
      for (uint32_t l = 0; l < nl; l++) {
        bool any = false;
        for (size_t i = 0; i < P; i++) {
          fmx_handle h = hs[i];                                  // (the launch macros refer to `h`)
          AlsState& a = h->als;
          const BlockRows& br = *h->slots[a.slot].blocks[r];
          AlsBlock& ab = a.blk[r];
          const uint32_t cnt = ab.level_ptr[l + 1] - ab.level_ptr[l];
          if (!cnt) continue;
          any = true;
          HIPCHK(h, hipSetDevice(h->device));
          hipStream_t st = h->stream;
          const double* lam = (f < 0) ? a.prior : a.prior + (size_t)(1 + f) * 2 * NG;
          const double* mu = lam + NG;
          float* param = (f < 0) ? h->tb.w : h->tb.V + f;
          const uint32_t pstride = (f < 0) ? h->tb.ws : h->tb.rs;
          const Shard sh = make_shard(h->cfg);
          double* delta = sharded ? ab.delta : nullptr;
#define FMX_REL_DRAW(ISV)                                                                                                                    \
          LANES_SWITCH(ab.lanes, FMX_LAUNCH_WAVES((k_rel_draw<ISV, LANES>), ((uint64_t)cnt * LANES + 63) / 64, st, br.rows.t_ent,              \
                       br.rows.seg_feat, br.rows.seg_rel, br.rows.nseg, (uint32_t)br.rows.nnz, ab.level_list + ab.level_ptr[l], cnt, param,    \
                       pstride, br.attr_offset, br.brow_ptr, B, ab.cache, opts->alpha, lam, mu, h->grp, opts->do_sample, opts->seed,           \
                       stream_id, sh, delta))
          if (f < 0) { FMX_REL_DRAW(false); } else { FMX_REL_DRAW(true); }
#undef FMX_REL_DRAW
          HIPCHK(h, hipGetLastError());
        }
        if (sharded && any) {
          std::vector<double*> bufs(P);
          for (size_t i = 0; i < P; i++) bufs[i] = hs[i]->als.blk[r].delta;
          int rc = group_allreduce_f64(g, bufs, (size_t)4 * B);
          if (rc) return rc;
          for (fmx_handle x : hs) {
            HIPCHK(x, hipSetDevice(x->device));
            hipLaunchKernelGGL(k_rel_apply_delta, gq, b1, 0, x->stream, x->als.blk[r].cache, x->als.blk[r].delta, B);
            HIPCHK(x, hipGetLastError());
          }
        }
      }
      for (fmx_handle x : hs) {
        AlsState& a = x->als;
        const BlockRows& br = *x->slots[a.slot].blocks[r];
        HIPCHK(x, hipSetDevice(x->device));
        if (f >= 0) hipLaunchKernelGGL((k_rel_sync<true>), g1, b1, 0, x->stream, br.map, N, B, (const double*)a.blk[r].cache, a.e);
        else        hipLaunchKernelGGL((k_rel_sync<false>), g1, b1, 0, x->stream, br.map, N, B, (const double*)a.blk[r].cache, a.e);
        HIPCHK(x, hipGetLastError());
      }
    }
    return FMX_OK;
  };
  const bool has_blocks = !h->slots[a0.slot].blocks.empty();
  if (h->cfg.k1) {                                         // draw_w per level, :454-476
    for (uint32_t l = 0; l < n_levels; l++) { int rc = level_step(l, -1); if (rc) return rc; }
    if (has_blocks) { int rc = block_steps(-1); if (rc) return rc; }
    for (fmx_handle x : hs) {
      HIPCHK(x, hipSetDevice(x->device));
      const dim3 gu((uint32_t)std::min<uint64_t>((x->n_local + 255) / 256, 2048));
      hipLaunchKernelGGL(k_als_unseen, gu, b1, 0, x->stream, x->als.seen, x->n_local, x->tb.w, x->tb.ws, x->als.prior, x->als.prior + NG, x->grp,
                         opts->do_sample, opts->seed, mcmc_stream(x->als.iter, MCMC_W_UNSEEN), make_shard(x->cfg));
    }
  }
  // the factors of the features with a training column, factor-major for the duration of the sweep (k_als_shadow)
  for (fmx_handle h : hs) {
    AlsState& a = h->als;
    const Slot& s = h->slots[a.slot];
    if (!a.vt || !s.nseg) continue;
    HIPCHK(h, hipSetDevice(h->device));
    KP_SWITCH(h->KP, hipLaunchKernelGGL((k_als_shadow<KP, true>), dim3(std::min<uint32_t>((s.nseg + 63) / 64, 4096)), dim3(256), 0, h->stream,
                                          a.level_list, s.seg_feat, s.nseg, h->tb, a.vt, a.vt_stride, (uint32_t)h->cfg.num_factor));
  }
  for (int f = 0; f < kf; f++) {                            // per factor: q_f is ready (k_als_eterms), draw_v per level :528-595
    for (fmx_handle x : hs) {
      HIPCHK(x, hipSetDevice(x->device));
      hipLaunchKernelGGL(k_als_load_q, g1, b1, 0, x->stream, x->als.e, x->als.q + (size_t)f * N, N);
    }
    for (uint32_t l = 0; l < n_levels; l++) { int rc = level_step(l, f); if (rc) return rc; }
    if (has_blocks) { int rc = block_steps(f); if (rc) return rc; }
  }
  for (fmx_handle h : hs) {
    AlsState& a = h->als;
    const Slot& s = h->slots[a.slot];
    HIPCHK(h, hipSetDevice(h->device));
    if (a.vt && s.nseg)
      KP_SWITCH(h->KP, hipLaunchKernelGGL((k_als_shadow<KP, false>), dim3(std::min<uint32_t>((s.nseg + 63) / 64, 4096)), dim3(256), 0, h->stream,
                                            a.level_list, s.seg_feat, s.nseg, h->tb, a.vt, a.vt_stride, (uint32_t)h->cfg.num_factor));
    if (kf > 0) {                                          // empty-row draws of every factor (:586-595) in one pass
      hipStream_t st = h->stream;
      KP_SWITCH(h->KP, FMX_LAUNCH_WAVES((k_als_unseen_v<KP>), (h->n_local + Map<KP>::EPI - 1) / Map<KP>::EPI, st, a.seen, h->n_local,
                                         h->tb, kf, a.prior, NG, h->grp, opts->do_sample, opts->seed,
                                         mcmc_stream(a.iter, MCMC_V_UNSEEN), make_shard(h->cfg)));
    }
    HIPCHK(h, hipGetLastError());
  }
  // full re-prediction (fm_learn_mcmc_simultaneous.h:122), train metric and new residuals (:139-196)
  {
    size_t bad = 0;
    int rc = als_repredict(hs, sharded ? g : nullptr, &bad);
    if (rc) { if (bad) h->err = hs[bad]->err; return rc; }
  }
  for (fmx_handle x : hs) {
    AlsState& a = x->als;
    const Slot& s = x->slots[a.slot];
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, hipMemsetAsync(x->acc, 0, 4 * sizeof(double), x->stream));
    hipLaunchKernelGGL(k_als_targets, g1, b1, 0, x->stream, a.e, s.target, N, x->cfg.task, x->cfg.min_target, x->cfg.max_target, x->acc,
                       opts->do_sample, opts->seed, mcmc_stream(a.iter, MCMC_TARGETS));
    HIPCHK(x, hipGetLastError());
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipMemcpyAsync(acc, h->acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
  for (fmx_handle x : hs) { HIPCHK(x, hipSetDevice(x->device)); HIPCHK(x, hipStreamSynchronize(x->stream)); x->als.iter++; }
  if (stats) {
    float ms = 0;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->device_seconds = ms * 1e-3;
    stats->levels = n_levels;
    stats->train_metric = (h->cfg.task == FMX_TASK_REGRESSION) ? std::sqrt(acc[0] / N) : acc[0] / N;
  }
  return FMX_OK;
}

// ---- fm_learn_mcmc over feature shards (fmx_group) --------------------------------------------------------------
int fmx_group_als_begin(fmx_group g, int train_slot) {
  if (!g) return FMX_E_ARG;
  for (fmx_handle x : g->hs) if (!x) return FMX_E_STATE;
  if (g->kind == GROUP_SINGLE) { int rc = fmx_als_begin(g->hs[0], train_slot); if (rc) g->err = g->hs[0]->err; return rc; }
  size_t bad = 0;
  const int rc = als_begin_shards(g->hs, g, train_slot, "fmx_group_als_begin", &bad);
  if (rc != FMX_OK) {                                                // a failed set-up leaves no session behind on any shard
    g->err = g->hs[bad]->err;
    for (fmx_handle y : g->hs) als_free(y);
  }
  return rc;
}

int fmx_group_als_sweep(fmx_group g, const fmx_als_opts* opts, fmx_als_stats* stats) {
  if (!g || !opts) return FMX_E_ARG;
  for (fmx_handle x : g->hs) if (!x) return FMX_E_STATE;
  int rc = als_sweep_shards(g->hs, g->kind == GROUP_SINGLE ? nullptr : g, opts, stats);
  if (rc) g->err = g->hs[0]->err;
  return rc;
}

// fmx_als_moments over the shards: the residual statistics are those of the (replicated) cache, the per-group parameter
// sums add up over the shards
int fmx_group_als_moments(fmx_group g, double* out) {
  if (!g || !out) return FMX_E_ARG;
  for (auto m : g->hs) if (!m) { g->err = "a member of the group was destroyed"; return FMX_E_STATE; }
  fmx_handle h = g->hs[0];
  const size_t cnt = 2 + 2 * (size_t)h->num_groups * (size_t)(1 + h->cfg.num_factor);
  std::vector<double> part(cnt);
  for (size_t i = 0; i < g->hs.size(); i++) {
    int rc = fmx_als_moments(g->hs[i], part.data());
    if (rc) { g->err = g->hs[i]->err; return rc; }
    if (i == 0) memcpy(out, part.data(), cnt * sizeof(double));
    else for (size_t c = 2; c < cnt; c++) out[c] += part[c];
  }
  return FMX_OK;
}

int fmx_group_als_end(fmx_group g) {
  if (!g) return FMX_E_ARG;
  for (fmx_handle x : g->hs) if (x) { int rc = fmx_als_end(x); if (rc) { g->err = x->err; return rc; } }
  return FMX_OK;
}

int fmx_als_sweep(fmx_handle h, const fmx_als_opts* opts, fmx_als_stats* stats) {
  if (!h || !opts) return FMX_E_ARG;
  { const int _sr = serve_refuse(h, "fmx_als_sweep"); if (_sr) return _sr; }
  if (h->cfg.shard_world > 1) return fail(h, FMX_E_STATE, "fmx_als_sweep on a feature shard: use fmx_group_als_sweep");
  return als_sweep_shards(std::vector<fmx_handle>(1, h), nullptr, opts, stats);
}

}  // extern "C"
