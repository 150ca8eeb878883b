"""GPU: AdaGrad and FTRL over feature shards (fmx_group_adapt_* / fmx_group_ftrl_* / fmx_group_param_sparsity).
All shards are loopback shards on device 0, built like make_group of tests/test_gpu_group.py; the one case on two distinct devices
(RCCL) skips where fewer than two are visible.

The references are the fp64 restatements libfm_amd/adaptive.py and libfm_amd/ftrl.py: the sharded rule IS the unsharded rule, because
the exchanged sums are the full sums -- only their association differs (per-shard partial sums, then the sum over the shards).  The
cases are tests/stateful_cases.py's seeds; the comparison is tests/test_gpu_stateful_fuzz.py's compare(): parameters at SC.RTOL /
SC.ATOL, every state table at rtol 1e-4 plus 8 x the fp32-vs-fp64 gap of the restatement, FTRL's zero pattern equal away from the
threshold (||z64| - l1| <= 1e-4 (1 + l1) excluded, at most max(2, 0.1 %) of a table).  tests/test_stateful_fuzz_cpu.py shows on the
CPU that every listed seed is inside that cap and that its fp32-vs-fp64 parameter gap leaves an 8 x allowance for another
association of the sums inside SC.ATOL; the shards' partial sums are such an association.

Every test prints its figures (compare() does) before it asserts."""
import numpy as np
import pytest

import datagen
import stateful_cases as SC
from oracle import oracle as O
from test_gpu_stateful_fuzz import ADAGRAD, PARITY, compare, same_bits

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -4
WORLDS = [(2, 0), (3, 1), (8, 1)]                               # (world, shard_hash)
# eight seeds of each list.  Between them (test_the_seeds_cover_the_named_edges): k = 0 (76; 79), widths off their padding (7: 17, 23: 65;
# 52: 33, 23: 65), 64 <= k <= 256 on rows a shard sees at most 12 entries of -- k_rowsums_multi (0, 1, 12, 23; 15, 12, 23), k0 off (1,
# 16; 36), k1 off (6, 16, 23; 23), a batch of 1 (0, 12; 12), a batch beyond the slot (1; 44), empty rows (6, 12; 12, 36, 44)
SEEDS = {"adagrad": (76, 7, 0, 1, 12, 6, 23, 16), "ftrl": (79, 15, 12, 23, 44, 36, 52, 2)}
NAMED = {"adagrad": ADAGRAD, "ftrl": PARITY}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def make_group(capi, world, devices, m, task, lr, lo, hi, shard_hash):
    hs = [capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, lo, hi, device=devices[r], shard_rank=r,
                      shard_world=world, shard_hash=shard_hash) for r in range(world)]
    grp = capi.Group(hs)
    grp.set_params(m.w0, m.w, m.v)
    return hs, grp


def close(hs, grp):
    grp.close()
    for h in hs:
        h.close()


def begin(drv, rule, opts):
    if rule == "adagrad":
        drv.adapt_begin("adagrad", opts["init_acc"], opts["eta"])
    else:
        drv.ftrl_begin(**opts)


def epoch(drv, rule, slot, batch, chunk):
    return (drv.adapt_epoch if rule == "adagrad" else drv.ftrl_epoch)(slot, batch, chunk)


def end(drv, rule):
    (drv.adapt_end if rule == "adagrad" else drv.ftrl_end)()


def state_rows(drv, rule, ids):
    if rule == "adagrad":
        nw, nv = drv.adapt_state_rows(ids)
        return {"n": (nw, nv)}
    zw, zv, nw, nv = drv.ftrl_state_rows(ids)
    return {"z": (zw, zv), "n": (nw, nv)}


def read(drv, rule, n):
    """(w0, w, v, {table: (linear weights' state, factors' state)}) through the group (or a handle): read() of the fuzz tests"""
    return tuple(drv.get_params()) + (state_rows(drv, rule, np.arange(n, dtype=np.uint32)),)


def restate(rule, m, d, task, lr, lo, hi, batch, chunk, opts, epochs):
    """`epochs` epochs of the restatement from model m, in fp64 and in fp32: ((m64, s64), (m32, s32))"""
    out = []
    for dt in (np.float64, np.float32):
        mm = m.copy()
        st = SC.new_state(rule, mm, opts)
        for _ in range(epochs):
            SC.rule_epoch(rule, mm, d, task, lr, lo, hi, batch, chunk, st, opts, dtype=dt)
        out.append((mm, st))
    return out


def run_sharded(capi, rule, c, world, shard_hash, epochs=SC.EPOCHS):
    hs, grp = make_group(capi, world, [0] * world, SC.start_model(c), c.task, SC.LR, c.lo, c.hi, shard_hash)
    try:
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        begin(grp, rule, c.opts(rule))
        stats = [epoch(grp, rule, 0, c.batch, c.chunk) for _ in range(epochs)]
        got = read(grp, rule, c.n)
        end(grp, rule)
        return got, stats
    finally:
        close(hs, grp)


# ---------------------------------------------------------------------------------------------
# 1. parity against the fp64 restatements
# ---------------------------------------------------------------------------------------------
def test_the_seeds_cover_the_named_edges():
    for rule in SC.RULES:
        own = SC.ADAGRAD_SEEDS if rule == "adagrad" else SC.FTRL_SEEDS
        assert len(SEEDS[rule]) >= 6 and set(SEEDS[rule]) <= set(own)
        cs = [SC.case(s) for s in SEEDS[rule]]
        rows = [len(c.y) for c in cs]
        lens = [np.diff(c.row_ptr.astype(np.int64)) for c in cs]
        assert any(c.k == 0 for c in cs)
        assert any(c.k % 16 not in (0,) and c.k > 16 for c in cs)                           # a width off its padding
        assert any(64 <= c.k <= 256 and l.mean() / 2 <= 12.0 for c, l in zip(cs, lens))     # short rows on every shard count: k_rowsums_multi
        assert any(not c.k0 for c in cs) and any(not c.k1 for c in cs)
        assert any(c.batch == 1 for c in cs) and any(c.batch > r for c, r in zip(cs, rows))
        assert any((l == 0).any() for l in lens)


@pytest.mark.parametrize("world, shard_hash", WORLDS)
@pytest.mark.parametrize("rule, seed", [(r, s) for r in SC.RULES for s in SEEDS[r]])
def test_sharded_epochs_are_the_restated_rule(capi, rule, seed, world, shard_hash):
    """two epochs of the seed's case over `world` loopback shards: parameters, every state row (read through the group) and FTRL's zero
    pattern against the fp64 restatement, by the fuzz tests' compare(); the stats carry the case's rows, batches, batch and micro-chunk.

    Measured on an MI355X: see the figures each case prints (gaps of v, w, w0 and of every state table with the absolute term in force);
    the largest ones stand in DESIGN.md section 26."""
    c, (m64, s64), (_, s32) = SC.restated(rule, seed)
    what = "%s world=%d hash=%d" % (c.describe(rule), world, shard_hash)
    print(what)
    assert SC.conditioning(rule, seed)["ok"], what
    got, stats = run_sharded(capi, rule, c, world, shard_hash)
    compare(got, rule, m64, s64, s32, what)
    rows = len(c.y)
    for es in stats:
        assert (es.rows, es.batches, es.batch_used, es.w0_chunk_used) == (rows, (rows + c.batch - 1) // c.batch, c.batch, c.chunk), what
    if not c.k0:
        assert got[0] == 0.0, what


# ---------------------------------------------------------------------------------------------
# 2. small edges of the owner on a shard
# ---------------------------------------------------------------------------------------------
EDGE_WORLD, EDGE_HASH = 8, 1
EDGE_N = EDGE_WORLD + 1


def edge_model(k):
    m = O.Model(EDGE_N, k, True, True, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, EDGE_N, max(k, 1), 0.05)[:k]
    m.w[:] = O.init_values(2, EDGE_N, 1, 0.02)[0]
    m.w0 = 0.03
    return m


def edge_rows(capi):
    """12 rows over world + 1 features, batch 4: the first batch names every feature (every shard has a segment, one shard two), the
    second only the features of two shards (nseg == 0 on the six others), the third holds an empty row and a feature repeated in a row"""
    owner, _ = capi.shard_place(EDGE_N, EDGE_WORLD, EDGE_HASH, np.arange(EDGE_N, dtype=np.uint32))
    assert sorted(np.bincount(owner, minlength=EDGE_WORLD).tolist()) == [1] * 7 + [2]       # most shards own one feature
    few = [int(j) for j in range(EDGE_N) if owner[j] in (owner[0], owner[1])]
    rng = np.random.default_rng(11)

    def row(ids):
        return [(int(j), float(np.round(rng.uniform(0.5, 1.5), 3))) for j in ids]
    rows = [row([0, 1, 2]), row([3, 4]), row([5, 6, 7]), row([8, 0]),
            row(few), row(few[:1]), row(few[::-1]), row(few[:1] * 2),
            [], row([2, 2, 5]), row([7]), row([8, 1, 3])]
    y = np.where(rng.random(len(rows)) < 0.5, 1.0, -1.0).astype(np.float32)
    return O.Data.from_rows(rows, y), owner, few


@pytest.mark.parametrize("rule", SC.RULES)
@pytest.mark.parametrize("k", [0, 5, 64])
def test_owner_edges_on_a_shard(capi, rule, k):
    """world + 1 features over 8 shards -- seven shards own ONE feature -- with a batch in which six shards own no feature of the batch
    (no segment there: the owner launch is skipped, the recurrence still runs), an empty row and an id repeated inside a row; then a slot
    of 0 rows: rows == 0 and nothing changes, bit for bit"""
    d, owner, few = edge_rows(capi)
    m, lr, batch, chunk, opts = edge_model(k), 0.01, 4, 2, NAMED[rule]
    (m64, s64), (_, s32) = restate(rule, m, d, 1, lr, -1.0, 1.0, batch, chunk, opts, 2)
    hs, grp = make_group(capi, EDGE_WORLD, [0] * EDGE_WORLD, m, 1, lr, -1.0, 1.0, EDGE_HASH)
    try:
        grp.upload_rows(0, d.entries, d.row_ptr, d.target)
        # the second batch (rows 4 .. 7) has entries on the shards of `few` only
        for r, h in enumerate(hs):
            ent, rp, _ = h.download_rows(0)
            assert (int(rp[8]) - int(rp[4]) > 0) == (r in (owner[0], owner[1]))
        begin(grp, rule, opts)
        for _ in range(2):
            es = epoch(grp, rule, 0, batch, chunk)
            assert (es.rows, es.batches, es.batch_used, es.w0_chunk_used) == (12, 3, 4, 2)
        got = read(grp, rule, EDGE_N)
        compare(got, rule, m64, s64, s32, "%s k=%d edges" % (rule, k))
        assert SC.gap(m64.w, m.w) > 1e-3                             # (the epochs moved the parameters far beyond the tolerances)
        grp.upload_rows(1, np.zeros(0, dtype=capi.ENTRY_DTYPE), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.float32))
        es = epoch(grp, rule, 1, batch, chunk)
        assert (es.rows, es.batches) == (0, 0)
        assert same_bits(got, read(grp, rule, EDGE_N))
        end(grp, rule)
    finally:
        close(hs, grp)


# ---------------------------------------------------------------------------------------------
# 3. bit reproducibility   4. a one-member group   5. batch = 0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule, seed", [("adagrad", 23), ("ftrl", 15)])
def test_two_sharded_runs_are_bit_identical(capi, rule, seed):
    c = SC.case(seed)
    a, _ = run_sharded(capi, rule, c, 4, 1)
    b, _ = run_sharded(capi, rule, c, 4, 1)
    assert same_bits(a, b)
    assert SC.gap(a[2], SC.start_model(c).v) > 1e-3


@pytest.mark.parametrize("rule, seed", [("adagrad", 7), ("ftrl", 2)])
def test_one_member_group_has_the_bits_of_the_handle(capi, rule, seed):
    """a group of one unsharded handle forwards to the per-handle calls: same parameters, same state, same stats"""
    c = SC.case(seed)
    m = SC.start_model(c)
    out = []
    for through_group in (False, True):
        h = capi.Handle(m.n, m.k, m.k0, m.k1, c.task, m.reg0, m.regw, m.regv, SC.LR, c.lo, c.hi)
        grp = capi.Group([h]) if through_group else None
        drv = grp if grp else h
        try:
            h.set_params(m.w0, m.w, m.v)
            h.upload_rows(0, c.entries, c.row_ptr, c.y)
            begin(drv, rule, c.opts(rule))
            stats = [epoch(drv, rule, 0, c.batch, c.chunk) for _ in range(2)]
            got = read(drv, rule, c.n)
            if grp:
                sp = grp.param_sparsity()
                assert (sp.features, sp.v_coords) == (c.n, c.n * c.k)
            end(drv, rule)
            out.append((got, [(s.rows, s.batches, s.batch_used, s.w0_chunk_used, s.max_feature_count) for s in stats]))
        finally:
            if grp:
                grp.close()
            h.close()
    assert same_bits(out[0][0], out[1][0]) and out[0][1] == out[1][1]


@pytest.mark.parametrize("rule", SC.RULES)
def test_batch_0_is_the_unsharded_handle_s_choice(capi, rule):
    """batch = 0 and w0_chunk = 0 over 8 shards resolve to what ONE unsharded handle chooses on the same rows (the collision mass summed
    over the shards): Criteo-shaped rows, whose frequent features cut the default"""
    e, rp, y, n = datagen.criteo_shaped(1500, 21, cat_ids=2000)
    m = O.Model(n, 8, True, True, 0.0, 0.0005, 0.001)
    m.v[:] = O.init_values(3, n, 8, 0.05)
    lr = 0.01
    h = capi.Handle(n, 8, True, True, 1, m.reg0, m.regw, m.regv, lr, -1.0, 1.0)
    try:
        h.set_params(m.w0, m.w, m.v)
        h.upload_rows(0, e, rp, y)
        begin(h, rule, NAMED[rule])
        one = epoch(h, rule, 0, 0, 0)
    finally:
        h.close()
    hs, grp = make_group(capi, 8, [0] * 8, m, 1, lr, -1.0, 1.0, 1)
    try:
        grp.upload_rows(0, e, rp, y)
        begin(grp, rule, NAMED[rule])
        many = epoch(grp, rule, 0, 0, 0)
    finally:
        close(hs, grp)
    print("batch_used %d / %d, w0_chunk_used %d / %d, collision mass %.6g / %.6g" % (
        many.batch_used, one.batch_used, many.w0_chunk_used, one.w0_chunk_used, many.collision_mass, one.collision_mass))
    assert (many.batch_used, many.w0_chunk_used, many.batches, many.rows) == (one.batch_used, one.w0_chunk_used, one.batches, one.rows)
    assert 1 <= one.batch_used < 1500 and one.w0_chunk_used == capi.default_w0_chunk(lr, 1)      # (the cut is in force: several batches)


# ---------------------------------------------------------------------------------------------
# 6. state rows   7. sparsity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule, seed", [("adagrad", 7), ("ftrl", 2)])
def test_state_rows_by_global_id_in_any_order(capi, rule, seed):
    """a permuted id list with repeats, fetched through the group, holds per position the restatement's value of THAT id, to case 1's
    tolerances; FTRL returns z before n"""
    c, (m64, s64), (_, s32) = SC.restated(rule, seed)
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.permutation(c.n), rng.integers(0, c.n, 40), [0, 0, c.n - 1, c.n - 1]]).astype(np.uint32)
    hs, grp = make_group(capi, 3, [0] * 3, SC.start_model(c), c.task, SC.LR, c.lo, c.hi, 1)
    try:
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        begin(grp, rule, c.opts(rule))
        for _ in range(SC.EPOCHS):
            epoch(grp, rule, 0, c.batch, c.chunk)
        dev = state_rows(grp, rule, ids)
        if rule == "ftrl":                                          # (the raw order of the binding's outputs: z_w, z_v, n_w, n_v)
            raw = grp.ftrl_state_rows(ids)
            assert np.array_equal(raw[0], dev["z"][0]) and np.array_equal(raw[2], dev["n"][0]) and (raw[2] >= 0).all() and (raw[0] < 0).any()
        assert code(capi, grp.adapt_state_rows if rule == "adagrad" else grp.ftrl_state_rows, np.array([1, c.n], dtype=np.uint32)) == E_ARG
    finally:
        close(hs, grp)
    ref = SC.tables(rule, s64)
    terms = {t: SC.ASSOC * g for t, g in SC.state_gaps(rule, s64, s32).items()}
    for t in ref:
        print("state rows %s %s: w %.3g v %.3g (absolute term %.3g)" % (rule, t, SC.gap(dev[t][0], ref[t][0][ids]), SC.gap(dev[t][1], ref[t][1][:, ids]), terms[t]))
        np.testing.assert_allclose(dev[t][0], ref[t][0][ids], rtol=SC.RTOL, atol=terms[t])
        np.testing.assert_allclose(dev[t][1], ref[t][1][:, ids], rtol=SC.RTOL, atol=terms[t])
    # a repeated id returns the same row at every position
    first = {}
    for p, j in enumerate(ids.tolist()):
        q = first.setdefault(j, p)
        for t in dev:
            assert dev[t][0][p] == dev[t][0][q] and np.array_equal(dev[t][1][:, p], dev[t][1][:, q])


SPARSITY_FIELDS = ("features", "w_zero", "v_coords", "v_zero", "v_zero_rows", "dead_features")


def test_group_sparsity_equals_the_unsharded_count(capi):
    """after a sharded FTRL run (seed 9: l1_w = 0.3 leaves 160 of 2784 linear weights at zero in the restatement) the parameters go,
    through get_param_rows over all ids, into one unsharded handle: fmx_group_param_sparsity equals its fmx_param_sparsity field for field"""
    seed = 9
    c, (m64, _), _ = SC.restated("ftrl", seed)
    assert c.k1 and (m64.w == 0).any() and (m64.w != 0).any()      # the restated model has zero AND non-zero linear weights
    hs, grp = make_group(capi, 3, [0] * 3, SC.start_model(c), c.task, SC.LR, c.lo, c.hi, 1)
    try:
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        begin(grp, "ftrl", c.opts("ftrl"))
        for _ in range(SC.EPOCHS):
            epoch(grp, "ftrl", 0, c.batch, c.chunk)
        sp = grp.param_sparsity()
        w, v = np.zeros(c.n), np.zeros((c.k, c.n))
        owner, _ = capi.shard_place(c.n, 3, 1, np.arange(c.n, dtype=np.uint32))
        for r, h in enumerate(hs):
            ids = np.flatnonzero(owner == r).astype(np.uint32)
            w[ids], v[:, ids] = h.get_param_rows(ids)
        w0 = hs[0].get_w0()
        for h in hs:                                                # the per-handle count keeps refusing a shard
            assert code(capi, h.param_sparsity) == E_UNSUPPORTED
    finally:
        close(hs, grp)
    m = SC.start_model(c)
    one = capi.Handle(c.n, c.k, c.k0, c.k1, c.task, m.reg0, m.regw, m.regv, SC.LR, c.lo, c.hi)
    try:
        one.set_params(w0, w, v)
        ref = one.param_sparsity()
    finally:
        one.close()
    print("sparsity: " + "  ".join("%s %d / %d" % (f, getattr(sp, f), getattr(ref, f)) for f in SPARSITY_FIELDS))
    for f in SPARSITY_FIELDS:
        assert getattr(sp, f) == getattr(ref, f), f
    assert 0 < sp.w_zero < sp.features == c.n


# ---------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------
def code(capi, fn, *args, **kw):
    with pytest.raises(capi.FmxError) as ei:
        fn(*args, **kw)
    return ei.value.code


def test_refusals_leave_the_group_as_it_was(capi):
    """every refusal returns its code before any launch: the parameters are the same bits after each, and the group trains afterwards.

    Not reachable, so not here: "a slot carrying row weights on a member" of a group of several shards.  fmx_set_row_weights refuses every
    feature shard and every group member, so no call sequence puts weights on such a slot; the driver checks Slot::weighted all the same
    (FMX_E_UNSUPPORTED), and a one-member group forwards to the per-handle epoch, which trains the weighted rule."""
    c = SC.case(7)
    m = SC.start_model(c)
    hs, grp = make_group(capi, 3, [0] * 3, m, c.task, SC.LR, c.lo, c.hi, 1)
    ids = np.arange(c.n, dtype=np.uint32)
    try:
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        start = grp.get_params()

        def unchanged():
            now = grp.get_params()
            return now[0] == start[0] and np.array_equal(now[1], start[1]) and np.array_equal(now[2], start[2])
        # before begin
        for rule in SC.RULES:
            assert code(capi, epoch, grp, rule, 0, 16, 4) == E_STATE
            assert code(capi, state_rows, grp, rule, ids) == E_STATE
            assert code(capi, end, grp, rule) == E_STATE
        # a begin that fails on its options opens a session on no member
        assert code(capi, grp.adapt_begin, "adagrad", -1.0, 0.0) == E_ARG
        assert code(capi, grp.adapt_begin, 7, 1.0, 0.0) == E_ARG
        assert code(capi, grp.ftrl_begin, alpha=0.05, beta=0.0, init_acc=0.0) == E_ARG
        assert "fmx_ftrl_begin: beta = 0 needs init_acc > 0" in capi.load().fmx_group_last_error(grp.g).decode()   # the per-handle message
        for rule in SC.RULES:
            assert code(capi, end, grp, rule) == E_STATE and code(capi, epoch, grp, rule, 0, 16, 4) == E_STATE
        # the other optimiser's session
        grp.adapt_begin()
        assert code(capi, grp.ftrl_begin, alpha=0.05) == E_STATE
        assert code(capi, grp.ftrl_epoch, 0, 16, 4) == E_STATE and code(capi, grp.ftrl_end) == E_STATE
        # the per-handle entry points keep refusing a member, session or not
        for h in hs:
            assert code(capi, h.adapt_begin) == E_UNSUPPORTED and code(capi, h.adapt_epoch, 0, 16, 4) == E_UNSUPPORTED
            assert code(capi, h.adapt_state_rows, ids[:1]) == E_UNSUPPORTED and code(capi, h.adapt_end) == E_UNSUPPORTED
        # slots: never uploaded, without targets, different row counts, kept relation blocks
        assert code(capi, grp.adapt_epoch, 5, 16, 4) == E_STATE
        grp.upload_rows(1, c.entries, c.row_ptr, None)
        assert code(capi, grp.adapt_epoch, 1, 16, 4) == E_STATE
        grp.upload_rows(2, c.entries, c.row_ptr, c.y)
        half = len(c.y) // 2
        hs[1].upload_rows(2, c.entries[:int(c.row_ptr[half])], c.row_ptr[:half + 1], c.y[:half])
        assert code(capi, grp.adapt_epoch, 2, 16, 4) == E_STATE
        be, br, _ = datagen.ragged_real(20, 4, 3, seed=62)
        rel = [(be, br, (np.arange(len(c.y)) % 4).astype(np.uint32), c.n - 20)]
        grp.upload_block_rows(3, c.entries, c.row_ptr, c.y, rel, keep=True)
        with pytest.raises(capi.FmxError) as ei:
            grp.adapt_epoch(3, 16, 4)
        assert ei.value.code == E_UNSUPPORTED and "relations are not supported with SGD" in ei.value.text
        # an open ALS / MCMC session on the members: the epoch, and a begin
        grp.als_begin(0)
        assert code(capi, grp.adapt_epoch, 0, 16, 4) == E_STATE
        assert code(capi, grp.adapt_begin) == E_STATE
        grp.als_end()
        assert unchanged()
        # the session works afterwards; after end the plain group epoch still trains
        es = grp.adapt_epoch(0, 16, 4)
        assert es.rows == len(c.y) and not unchanged()
        grp.adapt_end()
        assert code(capi, grp.adapt_end) == E_STATE
        grp.ftrl_begin(alpha=0.05)
        assert code(capi, grp.adapt_begin) == E_STATE
        grp.ftrl_end()
        before = grp.get_params()
        st = grp.sgd_epoch(0, capi.SGD_MINIBATCH, capi.APPLY_DEFAULT, 16, 4, capi.FLAG_BIAS_LAG, 1)
        assert st.rows == len(c.y) and SC.gap(grp.get_params()[2], before[2]) > 0
    finally:
        close(hs, grp)


def test_refusals_of_a_one_member_group(capi):
    """an SGDA session (only an unsharded handle can hold one) refuses the begin through its one-member group; a member that is a
    communicator rank is refused whatever it asks"""
    h = capi.Handle(100, 4, learn_rate=0.01)
    grp = capi.Group([h])
    try:
        h.sgda_begin()
        assert code(capi, grp.adapt_begin) == E_STATE and code(capi, grp.ftrl_begin, alpha=0.05) == E_STATE
        h.sgda_end()
        grp.adapt_begin()
        grp.adapt_end()
    finally:
        grp.close()
        h.close()
    hc = capi.Handle(100, 4, learn_rate=0.01)
    grp = None
    try:
        hc.comm_init_rank(capi.comm_unique_id(), 0, 1)
        grp = capi.Group([hc])
        assert code(capi, grp.adapt_begin) == E_UNSUPPORTED and code(capi, grp.ftrl_begin, alpha=0.05) == E_UNSUPPORTED
        assert code(capi, grp.adapt_epoch, 0, 16, 4) == E_UNSUPPORTED and code(capi, grp.param_sparsity) == E_UNSUPPORTED
    finally:
        if grp:
            grp.close()
        hc.close()


def test_destroying_members_with_an_open_session(capi):
    """the tables of an open session go with the member (fmx_destroy), whether or not the group was destroyed first"""
    c = SC.case(7)
    for group_first in (True, False):
        hs, grp = make_group(capi, 2, [0, 0], SC.start_model(c), c.task, SC.LR, c.lo, c.hi, 1)
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        grp.ftrl_begin(alpha=0.05)
        grp.ftrl_epoch(0, 16, 4)
        if group_first:
            grp.close()
        for h in hs[::-1]:
            h.close()
        grp.close()


# ---------------------------------------------------------------------------------------------
# 9. learner and command line
# ---------------------------------------------------------------------------------------------
def separable(capi, rows, seed):
    """a toy set a linear model separates (tests/test_gpu_query_eval.py): feature 0 .. 24 in positive rows, 25 .. 49 in negative ones"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(rows) < 0.4, 1.0, -1.0).astype(np.float32)
    ent = np.zeros(2 * rows, dtype=capi.ENTRY_DTYPE)
    ent["id"][0::2] = np.where(y > 0, rng.integers(0, 24, rows), rng.integers(25, 49, rows))
    ent["id"][1::2] = 49
    ent["value"] = 1.0
    return ent, np.arange(0, 2 * rows + 1, 2, dtype=np.uint64), y


def learner(L, optimizer, devices):
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = 50, 4
    l.fm.init(np.random.default_rng(3))
    l.task, l.num_iter, l.min_target, l.max_target = L.TASK_CLASSIFICATION, 3, -1.0, 1.0
    l.learn_rate, l.optimizer, l.devices, l.batch, l.w0_chunk = 0.05, optimizer, devices, 64, 8
    l.l1_w = 0.01
    l.extra_metrics = ("auc", "logloss")
    return l


@pytest.mark.parametrize("optimizer", ["adagrad", "ftrl"])
def test_learner_on_two_shards(capi, capsys, optimizer):
    """FMLearnSGD with devices = [0, 0] ends within case 1's tolerances of the same learner on one handle: model, predictions, the
    metrics of every iteration, set_queries' per-query AUC and sparsity()"""
    from libfm_amd import learner as L
    out = []
    for devices in (None, [0, 0]):
        tr, te = L.Data(*separable(capi, 200, 1)), L.Data(*separable(capi, 200, 2))
        l = learner(L, optimizer, devices)
        l.init()
        l.set_queries(te, np.random.default_rng(4).integers(0, 9, 200))
        l.learn(tr, te)
        assert (len(l._shards), type(l._h).__name__) == ((2, "Group") if devices else (0, "Handle"))
        sp = l.sparsity()
        out.append((l.fm.w0, l.fm.w.copy(), l.fm.v.copy(), l.predict(te), l.evaluate(te), l.evaluate_ex(te), l.evaluate_by_query(te).gauc,
                    [dict(r) for r in l.log], tuple(getattr(sp, f) for f in SPARSITY_FIELDS)))
        l.close()
        capsys.readouterr()
    one, two = out
    print("learner %s: w0 %.3g  w %.3g  v %.3g  predictions %.3g" % (optimizer, abs(one[0] - two[0]), SC.gap(one[1], two[1]), SC.gap(one[2], two[2]),
                                                                   SC.gap(one[3], two[3])))
    assert abs(one[0] - two[0]) <= SC.RTOL * abs(one[0]) + SC.ATOL
    np.testing.assert_allclose(two[1], one[1], rtol=SC.RTOL, atol=SC.ATOL)
    np.testing.assert_allclose(two[2], one[2], rtol=SC.RTOL, atol=SC.ATOL)
    np.testing.assert_allclose(two[3], one[3], rtol=SC.RTOL, atol=SC.ATOL)
    assert abs(one[4] - two[4]) * 200 <= 1 and abs(one[5].auc - two[5].auc) <= 1e-3 and abs(one[5].logloss - two[5].logloss) <= 1e-4
    assert abs(one[6] - two[6]) <= 1e-3
    for a, b in zip(one[7], two[7]):
        assert abs(a["logloss_test"] - b["logloss_test"]) <= 1e-4 and abs(a["rmse_train"] - b["rmse_train"]) * 200 <= 1
    assert one[8][0] == two[8][0] == 50 and one[8][2] == two[8][2] == 200
    assert np.abs(one[1]).max() > 1e-2                                                   # (trained: the linear weights started at 0)


def write_libfm(path, ent, rp, y):
    with open(path, "w") as f:
        for r in range(len(y)):
            f.write("%g %s\n" % (y[r], " ".join("%d:%g" % (e["id"], e["value"]) for e in ent[int(rp[r]):int(rp[r + 1])])))


@pytest.mark.parametrize("optimizer", ["adagrad", "ftrl"])
def test_cli_devices(capi, tmp_path, capsys, optimizer):
    """-devices 0,0 writes the -out of the run without the flag to 1e-4, under the same stdout lines"""
    from libfm_amd import cli
    trf, tef = str(tmp_path / "tr.libfm"), str(tmp_path / "te.libfm")
    write_libfm(trf, *separable(capi, 200, 1))
    write_libfm(tef, *separable(capi, 200, 2))
    outs = [str(tmp_path / "one.out"), str(tmp_path / "two.out")]
    argv = ["-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,4", "-iter", "3", "-method", "sgd", "-optimizer", optimizer, "-learn_rate", "0.05",
            "-init_stdev", "0.1", "-seed", "42", "-batch", "64"] + (["-l1", "0.01,0"] if optimizer == "ftrl" else [])
    assert cli.main(argv + ["-out", outs[0]]) == 0
    plain = capsys.readouterr()
    assert cli.main(argv + ["-out", outs[1], "-devices", "0,0"]) == 0
    sharded = capsys.readouterr()
    assert "ERROR" not in plain.err and "ERROR" not in sharded.err
    a, b = np.loadtxt(outs[0]), np.loadtxt(outs[1])
    print("cli %s: -out gap %.3g over %d rows" % (optimizer, SC.gap(a, b), len(a)))
    assert len(a) == 200 and a.std() > 1e-2
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-4)
    assert [x.split("\t")[0] for x in plain.out.splitlines()] == [x.split("\t")[0] for x in sharded.out.splitlines()]
    if optimizer == "ftrl":
        assert plain.err.count("sparsity\tfeatures=") == 1 == sharded.err.count("sparsity\tfeatures=")


# ---------------------------------------------------------------------------------------------
# 10. two distinct devices (RCCL)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule, seed", [("adagrad", 23)])
def test_two_devices_over_rccl(capi, rule, seed):
    """the same driver with one shard per GPU: the exchange is RCCL's all-reduce on the comm streams.  Skipped where fewer than two
    devices are visible (tests/test_gpu_group.py's pattern)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    c, (m64, s64), (_, s32) = SC.restated(rule, seed)
    hs, grp = make_group(capi, 2, [0, 1], SC.start_model(c), c.task, SC.LR, c.lo, c.hi, 1)
    try:
        grp.upload_rows(0, c.entries, c.row_ptr, c.y)
        begin(grp, rule, c.opts(rule))
        for _ in range(SC.EPOCHS):
            epoch(grp, rule, 0, c.batch, c.chunk)
        compare(read(grp, rule, c.n), rule, m64, s64, s32, c.describe(rule) + " over RCCL")
        end(grp, rule)
    finally:
        close(hs, grp)
