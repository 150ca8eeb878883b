// The level assignment of the ALS / MCMC set-up (libfm_amd/csrc/fmx_als_levels.h) against its definition, on the CPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/als_levels_check.cpp -o als_levels_check
//     ./als_levels_check
//
// 400 seeded column sets (up to 40 columns over up to 30 rows: empty columns, a row twice in one column, ids with gaps), each split
// over 1, 2, 3 and 5 "shards" the way the set-up hands them over -- shard after shard, a shard's columns in ITS order, which is
// the id order for one handle and for plain ownership and any order under the hashed one; some splits leave a shard without
// columns.  Every split must give the brute-force level per global id -- level(j) = 1 + max level of the smaller-id columns
// sharing a row with j -- and the same number of levels.
#include <cstdio>
#include <map>
#include <random>

#include "../libfm_amd/csrc/fmx_als_levels.h"

struct Ent { uint32_t e; float x; };                     // the layout of X^T's entries: (row, value)
struct Column { uint32_t gid; std::vector<uint32_t> rows; };

static std::map<uint32_t, uint32_t> brute(const std::vector<Column>& cols, uint32_t* n_levels) {
  std::map<uint32_t, uint32_t> level;
  *n_levels = 0;
  for (const Column& c : cols) {                         // (cols is in id order)
    uint32_t l = 0;
    for (const Column& d : cols) {
      if (d.gid >= c.gid) continue;
      bool share = false;
      for (uint32_t r : c.rows) for (uint32_t q : d.rows) share = share || r == q;
      if (share) l = std::max(l, level[d.gid] + 1);
    }
    level[c.gid] = l;
    *n_levels = std::max(*n_levels, l + 1);
  }
  return level;
}

int main() {
  std::mt19937_64 rng(20240607);
  auto upto = [&](uint32_t n) { return (uint32_t)(rng() % (n + 1)); };
  int checked = 0;
  for (int t = 0; t < 400; t++) {
    const uint32_t n_rows = 1 + upto(29), n_cols = upto(40);
    std::vector<Column> cols;
    uint32_t gid = upto(3);
    for (uint32_t j = 0; j < n_cols; j++, gid += 1 + upto(4)) {
      Column c{gid, {}};
      const uint32_t len = upto(5) == 0 ? 0 : 1 + upto(std::min<uint32_t>(n_rows, 6) - 1);
      for (uint32_t i = 0; i < len; i++) c.rows.push_back(upto(n_rows - 1));
      if (len && upto(3) == 0) c.rows.push_back(c.rows[0]);              // a row twice in one column
      cols.push_back(c);
    }
    uint32_t want_levels = 0;
    std::map<uint32_t, uint32_t> want = brute(cols, &want_levels);
    for (uint32_t P : {1u, 2u, 3u, 5u}) {
      const uint32_t mode = P == 1 ? 0 : upto(2);                        // 0: owner = id mod P; 1: hashed; 2: hashed, the last shard empty
      std::vector<std::vector<Column>> part(P);
      for (const Column& c : cols) {
        const uint32_t hsh = (uint32_t)((c.gid * 0x9E3779B97F4A7C15ull) >> 40);
        part[mode == 0 ? c.gid % P : hsh % (mode == 2 ? P - 1 : P)].push_back(c);
      }
      for (uint32_t i = 0; i < P; i++) if (mode) std::shuffle(part[i].begin(), part[i].end(), rng);
      std::vector<std::vector<Ent>> ent(P);
      std::vector<std::vector<uint32_t>> ids(P), first(P), level(P);
      std::vector<fmx::LevelCols<Ent>> parts;
      for (uint32_t i = 0; i < P; i++) {
        level[i].assign(part[i].size(), 0xFFFFFFFFu);
        for (const Column& c : part[i]) {
          ids[i].push_back(c.gid);
          first[i].push_back((uint32_t)ent[i].size());
          for (uint32_t r : c.rows) ent[i].push_back(Ent{r, 1.0f});
        }
        first[i].push_back((uint32_t)ent[i].size());
        parts.push_back({(uint32_t)part[i].size(), ids[i].data(), first[i].data(), ent[i].data(), level[i].data()});
      }
      const uint32_t got_levels = fmx::assign_levels(parts, n_rows);
      if (got_levels != want_levels) { printf("case %d, %u shards: %u levels, want %u\n", t, P, got_levels, want_levels); return 1; }
      for (uint32_t i = 0; i < P; i++)
        for (size_t j = 0; j < part[i].size(); j++)
          if (level[i][j] != want[part[i][j].gid]) {
            printf("case %d, %u shards: column %u has level %u, want %u\n", t, P, part[i][j].gid, level[i][j], want[part[i][j].gid]);
            return 1;
          }
      checked++;
    }
  }
  printf("als_levels_check: %d splits of 400 column sets agree with the definition\n", checked);
  return 0;
}
