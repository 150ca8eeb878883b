// fmx_als_levels.h -- the dependency levels of the columns an ALS / MCMC sweep visits.  Host only and free of HIP, so that
// scripts/als_levels_check.cpp can hold it against the definition under a sanitizer; fmx_als.hip (build_levels) is its one user.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fmx {

// the columns of X^T that one member holds, in its own order: column c has the GLOBAL feature id gid[c] and the entries
// ent[first[c]] .. ent[first[c + 1]] (Ent::e is the row); its level goes to level[c]
template <class Ent>
struct LevelCols { uint32_t n; const uint32_t* gid; const uint32_t* first; const Ent* ent; uint32_t* level; };

// level of column j = 1 + the largest level of the smaller-id columns that share a row with j (0 where there is none) -- so that
// "level by level, every member its columns of the level" is the reference's sequential sweep in id order.  Returns the number of
// levels.
template <class Ent>
uint32_t assign_levels(const std::vector<LevelCols<Ent>>& parts, uint32_t n_rows) {
  // ONE unsharded handle's columns arrive in id order (X^T of a single batch is sorted by feature, one segment per feature): they
  // are walked as they stand, nothing is copied or sorted.  Shards interleave; a feature has one owner and one segment there, so
  // equal ids do not occur -- and the stable sort would keep them in the order of arrival.
  struct Ref { uint32_t gid, part, col; };
  std::vector<Ref> order;
  const bool in_order = parts.size() == 1 && std::is_sorted(parts[0].gid, parts[0].gid + parts[0].n);
  if (!in_order) {
    for (size_t p = 0; p < parts.size(); p++)
      for (uint32_t c = 0; c < parts[p].n; c++) order.push_back(Ref{parts[p].gid[c], (uint32_t)p, c});
    std::stable_sort(order.begin(), order.end(), [](const Ref& a, const Ref& b) { return a.gid < b.gid; });
  }
  std::vector<uint32_t> rowlevel(std::max<uint32_t>(n_rows, 1), 0);      // 1 + the level of the last column that held the row
  uint32_t n_levels = 0;
  const auto visit = [&](const LevelCols<Ent>& p, uint32_t c) {
    uint32_t l = 0;
    for (uint32_t i = p.first[c]; i < p.first[c + 1]; i++) l = std::max(l, rowlevel[p.ent[i].e]);
    l += 1;
    for (uint32_t i = p.first[c]; i < p.first[c + 1]; i++) rowlevel[p.ent[i].e] = l;
    p.level[c] = l - 1;
    n_levels = std::max(n_levels, l);
  };
  if (in_order) for (uint32_t c = 0; c < parts[0].n; c++) visit(parts[0], c);
  else for (const Ref& r : order) visit(parts[r.part], r.col);
  return n_levels;
}

}  // namespace fmx
