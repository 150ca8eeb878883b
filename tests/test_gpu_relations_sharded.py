"""GPU: `-relation` blocks kept apart on feature shards (fmx_group_upload_block_rows_ex with FMX_BLOCKS_KEEP).  Every shard holds
the main rows restricted to its features and each block's rows restricted to the block attributes it owns -- nothing joined; the
sharded ALS / MCMC sweep (global block levels, one all-reduce of the cache changes per block level) and the group predict must be
the one-handle kept-block results, and ALS must land on the REAL reference's block-structured runs (fixtures rel_als_*).
Loopback shards on device 0."""
import io
import os
import subprocess

import numpy as np
import pytest

import datagen
from common import Golden
from conftest import ROOT, golden_cases

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness_gpu")
CASES = [c for c in golden_cases() if c.startswith("rel_als_")]


def _blocks_of(z):
    return [(z["rel%d_entries" % i], z["rel%d_row_ptr" % i], int(z["rel%d_num_feature" % i])) for i in range(int(z["n_relations"]))]


def _structured(n_users, n_items, n_rows, seed):
    """datagen.block_structured with the relations as upload_block_rows takes them, and num_attribute"""
    (ent, rp, y), blocks, maps = datagen.block_structured(n_users, n_items, n_rows, seed=seed)
    n_main, offs, o = 7, [], 7
    for _, _, nf in blocks:
        offs.append(o)
        o += nf
    return (ent, rp, y), [(be, bp, mp, off) for (be, bp, _), mp, off in zip(blocks, maps, offs)], o, n_main


def _shards(capi, n, k, world, shard_hash=1, **kw):
    hs = [capi.Handle(n, k, device=0, shard_rank=r, shard_world=world, shard_hash=shard_hash, **kw) for r in range(world)]
    return hs, capi.Group(hs)


def _close(*objs):
    for o in objs:
        o.close()


@pytest.mark.parametrize("world,shard_hash", [(2, 0), (2, 1), (3, 0), (3, 1), (5, 0), (5, 1)])
def test_nothing_joined_on_a_shard(world, shard_hash):
    """each shard's slot holds all N main rows and exactly the main entries it owns -- not its share of the joined table"""
    from libfm_amd import capi, sharding
    (ent, rp, y), rel, n, n_main = _structured(40, 25, 300, seed=5)
    hs, g = _shards(capi, n, 4, world, shard_hash)
    g.upload_block_rows(0, ent, rp, y, rel, keep=True)
    nfs = np.diff([off for _, _, _, off in rel] + [n])
    flat_ent, flat_rp, _ = datagen.expand_blocks(ent, rp, [(be, bp, nf) for (be, bp, _, _), nf in zip(rel, nfs)], [mp for _, _, mp, _ in rel], n_main)
    for r, h in enumerate(hs):
        got_ent, got_rp, got_y = h.download_rows(0)
        want_ent, want_rp = sharding.filter_rows(ent, rp, r, world, n, shard_hash)
        joined, _ = sharding.filter_rows(flat_ent, flat_rp, r, world, n, shard_hash)
        assert len(got_rp) == 301 and np.array_equal(got_y, y)
        assert np.array_equal(got_rp, want_rp) and np.array_equal(got_ent, want_ent)
        assert len(got_ent) < len(joined)
    _close(g, *hs)


def _random_params(oracle, n, k, seed, scale=0.3):
    m = oracle.Model(n, k, True, True, 0.0, 0.0, 0.0)
    m.v[:] = oracle.init_values(seed, n, k, scale)
    m.w[:] = oracle.init_values(seed + 1, n, 1, scale)[0]
    m.w0 = 0.25
    return m


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n_rows", [300, 300000])
def test_group_predict_on_kept_blocks(oracle, world, n_rows):
    """group predict / evaluate on kept blocks = one-handle kept-block predict = the oracle on the expanded rows; 300 000 rows
    cross the 262 144-row chunk of fmx_group_predict"""
    from libfm_amd import capi
    (ent, rp, y), rel, n, _ = _structured(40 if n_rows < 1000 else 3000, 25 if n_rows < 1000 else 800, n_rows, seed=11)
    k = 8
    m = _random_params(oracle, n, k, 3)
    lo, hi = float(y.min()), float(y.max())
    one = capi.Handle(n, k, True, True, 0, 0, 0, 0, 0.0, lo, hi, device=0)
    one.set_params(m.w0, m.w, m.v)
    one.upload_block_rows(0, ent, rp, y, rel, keep=True)
    one.upload_block_rows(1, ent, rp, y, rel, keep=False)
    flat_ent, flat_rp, _ = one.download_rows(1)
    want = oracle.predict_raw(m, oracle.Data(flat_ent, flat_rp, y))
    p1 = one.predict(0, n_rows)
    hs, g = _shards(capi, n, k, world, 1, min_target=lo, max_target=hi)
    g.set_params(m.w0, m.w, m.v)
    g.upload_block_rows(0, ent, rp, y, rel, keep=True)
    pg = g.predict(0, n_rows)
    np.testing.assert_allclose(pg, p1, rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(pg, want, rtol=1e-4, atol=5e-5)
    assert abs(g.evaluate(0).rmse - one.evaluate(0).rmse) < 1e-5
    _close(g, *hs)
    one.close()


def _learner(L, D, g, z, oracle, devices, keep=True, iters=None, sample=False):
    fm = L.FMModel()
    fm.num_attribute, fm.num_factor, fm.k0, fm.k1 = g.n, g.k, bool(g.k0), bool(g.k1)
    fm.reg0, fm.regw, fm.regv = g.reg
    m = g.model(oracle, "init")
    fm.w0, fm.w, fm.v = m.w0, m.w.copy(), m.v.copy()
    l = L.FMLearnALS()
    l.fm, l.task, l.num_iter, l.min_target, l.max_target = fm, g.task, iters or g.iters, g.min_target, g.max_target
    if sample:
        l.w_lambda, l.v_lambda, l.do_sample, l.seed = 2.0, 3.0, True, 1234
    else:
        l.w_lambda, l.v_lambda = g.reg[1], g.reg[2]
        if "group" in z.files:
            l.groups, l.w_lambda, l.v_lambda = z["group"], z["w_lambda_g"], z["v_lambda_g"]
    l.devices = devices
    l.out = io.StringIO()
    train = L.Data(z["train_entries"], z["train_row_ptr"], g.train_target)
    test = L.Data(z["test_entries"], z["test_row_ptr"], g.test_target)
    off = int(z["n_main"])
    for i, (be, bp, nf) in enumerate(_blocks_of(z)):
        rel = D.Relation(be, bp, nf)
        train.add_relation(rel, z["rel%d_train" % i], off)
        test.add_relation(rel, z["rel%d_test" % i], off)
        off += nf
    train.keep_blocks = test.keep_blocks = keep
    l.init()
    l.learn(train, test)
    return l, test


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
@pytest.mark.parametrize("name", CASES)
def test_sharded_als_on_kept_blocks_matches_reference(oracle, name, devices):
    """FMLearnALS over loopback shards with the blocks kept apart lands on the real reference's run (tolerances of
    test_als_on_relations_matches_reference)"""
    from libfm_amd import data as D
    from libfm_amd import learner as L
    g = Golden(name)
    z = g.z
    l, test = _learner(L, D, g, z, oracle, devices)
    assert len(l._shards) == len(devices)
    assert abs(l.fm.w0 - float(z["final_w0"])) <= 1e-4 * abs(float(z["final_w0"])) + 2e-5
    np.testing.assert_allclose(l.fm.w, z["final_w"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(l.fm.v, z["final_v"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(l.predict(test), z["pred_out"], rtol=1e-4, atol=5e-5)
    l.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_sampled_chain_on_sharded_kept_blocks(oracle, devices):
    """do_sample = 1: the noise of a block attribute is keyed by its GLOBAL id, so three sampled sweeps over the shards are the
    one-handle kept-block chain of the same seed"""
    from libfm_amd import data as D
    from libfm_amd import learner as L
    g = Golden("rel_als_reg")
    z = g.z
    res = []
    for dv in (None, devices):
        l, test = _learner(L, D, g, z, oracle, dv, iters=3, sample=True)
        res.append((l.fm.w0, l.fm.w.copy(), l.fm.v.copy(), l.predict(test).copy()))
        l.close()
    (w0a, wa, va, pa), (w0b, wb, vb, pb) = res
    assert np.abs(va - g.model(oracle, "init").v).max() > 0.05                                # the chain moved
    assert abs(w0a - w0b) <= 1e-4 * abs(w0a) + 2e-5
    np.testing.assert_allclose(wb, wa, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(vb, va, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pb, pa, rtol=1e-4, atol=1e-4)


def _random_relational(seed, n_rel, repeats=False):
    """main rows (1..3 of 12 attributes) + n_rel blocks with ragged rows: empty block rows, block rows no main row maps to,
    a block of 1 or 2 attributes (fewer than shards); repeats: ids repeated inside a block row (predict only)"""
    rng = np.random.default_rng(seed)
    N, n_main = 400, 12
    ids = [list(rng.choice(n_main, rng.integers(1, 4), replace=False)) for _ in range(N)]
    ent, rp, _ = datagen._pack(ids, [list(rng.uniform(0.5, 1.5, len(r))) for r in ids], np.zeros(N))
    y = rng.integers(1, 6, N).astype(np.float32)
    rel, off = [], n_main
    for r in range(n_rel):
        nf = [1, 2, 23][r % 3]
        B = int(rng.integers(20, 60))
        rows_i, rows_v = [], []
        for b in range(B):
            sz = 0 if b % 7 == 3 else int(rng.integers(1, min(nf, 4) + 1))
            ri = list(rng.choice(nf, sz, replace=False))
            if repeats and sz and b % 5 == 0:
                ri = ri + [ri[0]]
            rows_i.append(ri)
            rows_v.append(list(rng.uniform(-1.0, 1.0, len(ri))))
        be, bp, _ = datagen._pack(rows_i, rows_v, np.zeros(B))
        used = rng.choice(B, max(B * 2 // 3, 1), replace=False)             # the other block rows: no main row maps to them
        rel.append((be, bp, rng.choice(used, N).astype(np.uint32), off))
        off += nf
    return (ent, rp, y), rel, off


EDGE = [(1, 2, 1, 1, True, 1), (2, 3, 2, 8, False, 2), (3, 3, 3, 17, True, 3), (4, 2, 2, 64, True, 1), (5, 3, 1, 8, True, 3),
        (6, 2, 3, 17, False, 2)]


@pytest.mark.parametrize("seed,world,n_rel,k,k1,G", EDGE)
def test_sharded_kept_blocks_edge_cases(oracle, seed, world, n_rel, k, k1, G):
    """two sweeps + predict over the shards = the one-handle kept path (1e-4), on blocks with fewer attributes than shards,
    unmapped and empty block rows, 1 - 3 relations, k in {1, 8, 17, 64}, k1 off, 1 - 3 attribute groups"""
    from libfm_amd import capi
    (ent, rp, y), rel, n = _random_relational(seed, n_rel)
    rng = np.random.default_rng(seed + 100)
    groups = rng.integers(0, G, n).astype(np.uint32) if G > 1 else None
    if groups is not None:
        groups[:G] = np.arange(G)
    m = _random_params(oracle, n, k, seed + 7, 0.1)
    lo, hi = float(y.min()), float(y.max())
    kw = dict(k0=True, k1=k1, task=0, reg0=0.1, regw=1.0, regv=2.0, min_target=lo, max_target=hi)
    one = capi.Handle(n, k, device=0, **kw)
    hs, g = _shards(capi, n, k, world, seed % 2, **kw)
    out = []
    for x, members in ((one, [one]), (g, hs)):
        for h in members:
            h.set_groups(groups)
        x.set_params(m.w0, m.w, m.v)
        x.upload_block_rows(0, ent, rp, y, rel, keep=True)
        x.als_begin(0)
        for _ in range(2):
            x.als_sweep(1.5, 2.5)
        x.als_end()
        w0, w, v = x.get_params()
        out.append((w0, w.copy(), v.copy(), x.predict(0, len(y))))
    (w0a, wa, va, pa), (w0b, wb, vb, pb) = out
    assert abs(w0a - w0b) <= 1e-4 * abs(w0a) + 2e-5
    np.testing.assert_allclose(wb, wa, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(vb, va, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(pb, pa, rtol=1e-4, atol=5e-5)
    _close(g, *hs)
    one.close()


@pytest.mark.parametrize("seed,world", [(7, 2), (8, 3)])
def test_sharded_kept_blocks_predict_with_repeated_ids(oracle, seed, world):
    """ids repeated inside a block row: predict only (the ALS sweeps of test_gpu_fuzz.py keep such rows out too)"""
    from libfm_amd import capi
    (ent, rp, y), rel, n = _random_relational(seed, 3, repeats=True)
    k = 8
    m = _random_params(oracle, n, k, seed, 0.3)
    one = capi.Handle(n, k, device=0)
    one.set_params(m.w0, m.w, m.v)
    one.upload_block_rows(0, ent, rp, y, rel, keep=True)
    hs, g = _shards(capi, n, k, world, 1)
    g.set_params(m.w0, m.w, m.v)
    g.upload_block_rows(0, ent, rp, y, rel, keep=True)
    np.testing.assert_allclose(g.predict(0, len(y)), one.predict(0, len(y)), rtol=1e-4, atol=5e-5)
    _close(g, *hs)
    one.close()


def test_group_sgd_refuses_kept_blocks():
    from libfm_amd import capi
    (ent, rp, y), rel, n, _ = _structured(40, 25, 300, seed=5)
    hs, g = _shards(capi, n, 4, 2, 1, learn_rate=0.01)
    g.upload_block_rows(0, ent, rp, y, rel, keep=True)
    with pytest.raises(capi.FmxError) as ei:
        g.sgd_epoch(0, capi.SGD_MINIBATCH)
    assert ei.value.code == -4 and "not supported with SGD" in ei.value.text       # FMX_E_UNSUPPORTED, fm_learn_sgd.h:61-63
    _close(g, *hs)


@pytest.mark.parametrize("blocks", ["keep", "expand"])
def test_reference_driver_on_sharded_relations(oracle, tmp_path, blocks):
    """the reference's own loaders with `-relation` and gpu_devices = 0,0: adapter/fm_learn_mcmc_gpu.h uploads through
    fmx_group_upload_block_rows_ex and honours gpu_blocks_expand; both land on the stock block-structured learner"""
    if not os.path.exists(HARNESS):
        pytest.skip("oracle/_ref/ref_harness_gpu not built (needs /root/reference at build time)")
    from libfm_amd import data as D
    O = oracle
    g = Golden("rel_als_cls_groups")
    z = g.z
    td = str(tmp_path)
    trf, tef, pre = os.path.join(td, "train.libfm"), os.path.join(td, "test.libfm"), os.path.join(td, "out")
    O.Data(z["train_entries"], z["train_row_ptr"], z["train_target"]).write_libsvm(trf)
    O.Data(z["test_entries"], z["test_row_ptr"], z["test_target"]).write_libsvm(tef)
    names = []
    for i in range(int(z["n_relations"])):
        px = os.path.join(td, "rel%d" % i)
        be, bp, nf = z["rel%d_entries" % i], z["rel%d_row_ptr" % i], int(z["rel%d_num_feature" % i])
        et, cp = D.transpose(be, bp, nf)
        D.write_binary_matrix(px + ".xt", et, cp, num_cols=len(bp) - 1)
        np.savetxt(px + ".train", z["rel%d_train" % i], fmt="%d")
        np.savetxt(px + ".test", z["rel%d_test" % i], fmt="%d")
        np.savetxt(px + ".groups", z["rel%d_groups" % i], fmt="%d")
        names.append(px)
    env = dict(os.environ, FMX_RELATIONS=",".join(names), FMX_GPU_BLOCKS=blocks, FMX_GPU_DEVICES="0,0",
               FMX_GROUP_REG=",".join(repr(float(x)) for x in list(z["w_lambda_g"]) + list(z["v_lambda_g"])))
    cfg = ["als_gpu", trf, tef, str(z["task"]), int(z["k0"]), int(z["k1"]), int(z["k"]), int(z["iters"]),
           repr(g.reg[0]), repr(g.reg[1]), repr(g.reg[2]), repr(float(z["init_stdev"])), int(z["seed"]), pre]
    r = subprocess.run([HARNESS] + [str(c) for c in cfg], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    final = O.Model.from_dump(pre + ".final.bin")
    pred_out = np.fromfile(pre + ".pred_out.bin", dtype=np.float64)
    np.testing.assert_allclose(final.v, z["final_v"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(final.w, z["final_w"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pred_out, z["pred_out"], rtol=1e-4, atol=1e-4)
