#!/usr/bin/env python3
"""Generate tests/golden/bpr_*.npz: the pairwise ranking learner (include/fmx.h, "pairwise ranking") run by the REAL reference's
fm_model::predict and fm_pairSGD (fm_sgd.h:53-126).

No learner of the reference calls fm_pairSGD, so the loop around it is a small harness of ours (HARNESS below): it includes the
reference's headers (Data.h first: it defines DATA_FLOAT, Data.h:31, which fm_sgd.h uses), starts from fm.init() after
srand(seed), and per pair computes y_a, y_b with fm.predict, mult = -(1 - sigmoid(y_a - y_b)) and calls fm_pairSGD.  It records
the parameters at the start, after epoch 1 and after the last epoch, and the raw predictions of the test rows.

Needs the reference sources and g++ (build container only); the GPU tests read only the committed .npz files.

    python tests/golden/make_bpr_golden.py [--ref /path/to/reference]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import datagen  # noqa: E402

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "util/util.h"
#include "libfm/src/Data.h"
#include "fm_core/fm_sgd.h"

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}
struct Rows {
  std::vector<uint64_t> rp;
  std::vector<sparse_entry<DATA_FLOAT> > e;
  sparse_row<DATA_FLOAT> row(uint32_t r) {
    sparse_row<DATA_FLOAT> x;
    x.data = e.empty() ? NULL : &e[0] + rp[r];
    x.size = (uint)(rp[r + 1] - rp[r]);
    return x;
  }
};
static void rd_rows(FILE* f, Rows& R) {
  uint32_t n; uint64_t nnz;
  rd(f, &n, 1); rd(f, &nnz, 1);
  R.rp.resize(n + 1); rd(f, &R.rp[0], n + 1);
  R.e.resize(nnz);
  for (uint64_t i = 0; i < nnz; i++) { uint32_t id; float v; rd(f, &id, 1); rd(f, &v, 1); R.e[i].id = id; R.e[i].value = v; }
}
static void dump(FILE* o, fm_model& fm) {
  fwrite(&fm.w0, 8, 1, o);
  for (uint j = 0; j < fm.num_attribute; j++) { double w = fm.w(j); fwrite(&w, 8, 1, o); }
  for (int f = 0; f < fm.num_factor; f++)
    for (uint j = 0; j < fm.num_attribute; j++) { double v = fm.v(f, j); fwrite(&v, 8, 1, o); }
}
int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: bpr_harness <in> <out>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hdr[7]; rd(f, hdr, 7);            // n, k, k0, k1, iters, seed, set_w0
  double cfg[6]; rd(f, cfg, 6);             // lr, reg0, regw, regv, init_stdev, w0
  Rows tr, te;
  rd_rows(f, tr);
  uint64_t P; rd(f, &P, 1);
  std::vector<uint32_t> pa(P + 1), pb(P + 1);
  rd(f, &pa[0], P); rd(f, &pb[0], P);
  rd_rows(f, te);
  fclose(f);
  fm_model fm;
  fm.num_attribute = (uint)hdr[0];
  fm.num_factor = (int)hdr[1];
  fm.k0 = hdr[2] != 0; fm.k1 = hdr[3] != 0;
  fm.reg0 = cfg[1]; fm.regw = cfg[2]; fm.regv = cfg[3];
  fm.init_mean = 0.0; fm.init_stdev = cfg[4];
  srand((unsigned)hdr[5]);
  fm.init();
  if (hdr[6]) fm.w0 = cfg[5];
  FILE* o = fopen(argv[2], "wb");
  dump(o, fm);
  const int k = fm.num_factor;
  DVector<double> sum_pos(k), sum_neg(k), sum_sqr(k), grad(fm.num_attribute);
  DVector<bool> grad_visited(fm.num_attribute);
  const double lr = cfg[0];
  for (int64_t it = 0; it < hdr[4]; it++) {
    for (uint64_t t = 0; t < P; t++) {
      sparse_row<DATA_FLOAT> xa = tr.row(pa[t]), xb = tr.row(pb[t]);
      double ya = fm.predict(xa, sum_pos, sum_sqr);
      double yb = fm.predict(xb, sum_neg, sum_sqr);
      double mult = -(1.0 - sigmoid(ya - yb));
      fm_pairSGD(&fm, lr, xa, xb, mult, sum_pos, sum_neg, grad_visited, grad);
    }
    if (it == 0) dump(o, fm);
  }
  dump(o, fm);
  for (uint32_t r = 0; r + 1 < te.rp.size(); r++) {
    sparse_row<DATA_FLOAT> x = te.row(r);
    double y = fm.predict(x, sum_pos, sum_sqr);
    fwrite(&y, 8, 1, o);
  }
  fclose(o);
  return 0;
}
"""


def _pack(ids, vals):
    lens = [len(r) for r in ids]
    rp = np.zeros(len(ids) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    ent = np.zeros(int(rp[-1]), dtype=[("id", np.uint32), ("value", np.float32)])
    ent["id"] = [j for r in ids for j in r]
    ent["value"] = [x for r in vals for x in r]
    return ent, rp


def ml_negatives(n_users, n_items, n_pos, seed, zipf=0.0):
    """MovieLens-shaped implicit feedback: user one-hot + item one-hot rows.  Every observed (u, i) row is followed by a row (u, j) with
    a sampled item j the user has not seen; the pair says (u, i) is preferred to (u, j).  zipf > 0: item popularity ~ rank^-zipf, and
    user 0 is a heavy user (a third of the observations)."""
    rng = np.random.default_rng(seed)
    if zipf > 0:
        p = 1.0 / np.arange(1, n_items + 1) ** zipf
        p /= p.sum()
        items = rng.choice(n_items, n_pos, p=p)
        users = np.where(rng.random(n_pos) < 1 / 3, 0, rng.integers(0, n_users, n_pos))
    else:
        users, items = rng.integers(0, n_users, n_pos), rng.integers(0, n_items, n_pos)
    seen = set(zip(users.tolist(), items.tolist()))
    ids, vals, pa, pb = [], [], [], []
    for u, i in zip(users.tolist(), items.tolist()):
        j = int(rng.integers(0, n_items))
        while (u, j) in seen:
            j = int(rng.integers(0, n_items))
        pa.append(len(ids)); ids.append([u, n_users + i]); vals.append([1.0, 1.0])
        pb.append(len(ids)); ids.append([u, n_users + j]); vals.append([1.0, 1.0])
    ent, rp = _pack(ids, vals)
    return ent, rp, np.array(pa, np.uint32), np.array(pb, np.uint32)


def ragged_pairs(n_features, n_rows, n_pairs, max_nnz, seed):
    """ragged real-valued rows with ids repeated inside a row (datagen.ragged_real duplicates=True) over a small id space, so that
    x_a and x_b of a pair often share ids; random pairs, some of them rows next to each other"""
    ent, rp, _ = datagen.ragged_real(n_features, n_rows, max_nnz, seed, duplicates=True)
    rng = np.random.default_rng(seed + 1)
    pa = rng.integers(0, n_rows, n_pairs).astype(np.uint32)
    pb = rng.integers(0, n_rows, n_pairs).astype(np.uint32)
    return ent, rp, pa, pb


CASES = {
    # MovieLens-shaped one-hot user / item rows with sampled negatives, k = 8
    "bpr_ml_k8": dict(data=lambda: ml_negatives(100, 60, 900, 101), test=lambda: ml_negatives(100, 60, 60, 102),
                      n=160, k=8, k0=1, k1=1, iters=5, lr=0.05, reg=(0.0, 0.001, 0.01), init_stdev=0.1, seed=11),
    # ragged real values, ids repeated inside a row and shared by x_a and x_b, k = 5
    "bpr_ragged_dup_k5": dict(data=lambda: ragged_pairs(40, 200, 500, 9, 201), test=lambda: ragged_pairs(40, 50, 1, 9, 202),
                              n=40, k=5, k0=1, k1=1, iters=4, lr=0.02, reg=(0.0, 0.01, 0.02), init_stdev=0.1, seed=12),
    # k0 = 1 with reg0 > 0 (w0 decays, fm_sgd.h:56) and no linear terms; fm.init() leaves w0 = 0, so w0 = 0.5 first
    "bpr_w0_nolin_k4": dict(data=lambda: ml_negatives(50, 40, 400, 301), test=lambda: ml_negatives(50, 40, 40, 302),
                            n=90, k=4, k0=1, k1=0, iters=3, lr=0.05, reg=(0.01, 0.0, 0.005), init_stdev=0.1, seed=13, w0=0.5),
    # Zipf items at k = 64, user 0 with far more than 64 pairs
    "bpr_zipf_k64": dict(data=lambda: ml_negatives(16, 72, 300, 401, zipf=1.1), test=lambda: ml_negatives(16, 72, 30, 402, zipf=1.1),
                         n=88, k=64, k0=1, k1=1, iters=3, lr=0.05, reg=(0.0, 0.001, 0.001), init_stdev=0.05, seed=14),
}


def _write_rows(f, ent, rp):
    np.array([len(rp) - 1], np.uint32).tofile(f)
    np.array([len(ent)], np.uint64).tofile(f)
    rp.astype(np.uint64).tofile(f)
    ent.tofile(f)


def run_case(exe, name, c, tmp):
    ent, rp, pa, pb = c["data"]()
    tent, trp, _, _ = c["test"]()
    n, k = c["n"], c["k"]
    assert int(ent["id"].max()) < n and int(tent["id"].max()) < n
    inp, out = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
    with open(inp, "wb") as f:
        np.array([n, k, c["k0"], c["k1"], c["iters"], c["seed"], 1 if "w0" in c else 0], np.int64).tofile(f)
        np.array([c["lr"], *c["reg"], c["init_stdev"], c.get("w0", 0.0)], np.float64).tofile(f)
        _write_rows(f, ent, rp)
        np.array([len(pa)], np.uint64).tofile(f)
        pa.tofile(f)
        pb.tofile(f)
        _write_rows(f, tent, trp)
    subprocess.check_call([exe, inp, out])
    raw = np.fromfile(out, np.float64)
    per = 1 + n + k * n
    sets = [raw[i * per:(i + 1) * per] for i in range(3)]
    pred = raw[3 * per:]
    assert len(pred) == len(trp) - 1
    z = dict(n=n, k=k, k0=c["k0"], k1=c["k1"], iters=c["iters"], lr=c["lr"], reg=np.array(c["reg"]),
             train_entries=ent, train_row_ptr=rp, pair_a=pa, pair_b=pb, test_entries=tent, test_row_ptr=trp, test_pred=pred)
    for tag, p in zip(("init", "epoch1", "final"), sets):
        z[tag + "_w0"] = p[0]
        z[tag + "_w"] = p[1:1 + n]
        z[tag + "_v"] = p[1 + n:].reshape(k, n)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **z)
    print("%-20s %5d pairs  %7d bytes" % (name, len(pa), os.path.getsize(path)))


def main():
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else "/root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "bpr_harness.cpp"), os.path.join(tmp, "bpr_harness")
        with open(src, "w") as f:
            f.write(HARNESS)
        subprocess.check_call(["g++", "-O2", "-w", "-I" + os.path.join(ref, "src"), "-o", exe, src])
        for name, c in CASES.items():
            run_case(exe, name, c, tmp)


if __name__ == "__main__":
    main()
