"""GPU: the two optimisers that keep per-coordinate state on the minibatch rule -- AdaGrad (fmx_adapt_*, k_adapt_apply_seg) and
FTRL-proximal (fmx_ftrl_*, k_ftrl_apply_seg), both stateful_seg_block under the driver stateful_epoch -- on seeded random shapes, at
the named edges of the owner block and through session orders, against the float64 restatements libfm_amd/adaptive.py and
libfm_amd/ftrl.py.  tests/test_gpu_adagrad.py and tests/test_gpu_ftrl.py hold the same kernels at essentially one data shape (32
entries in every row, batch 64, micro-chunk 16); here the rows are ragged with empty ones and repeated ids, the batches divide nothing,
the widths sit on both sides of every padding boundary, and the session changes its batch, its slot, its parameters and its options
under a live state.  The cases and their seeds are tests/stateful_cases.py's; tests/test_stateful_fuzz_cpu.py establishes on the CPU
that every seed is well-conditioned.

Tolerances (the project's, tests/test_gpu_ftrl.py): parameters rtol 1e-4 / atol 2e-5.  Every state table (AdaGrad's n; FTRL's z and n)
rtol 1e-4 plus an absolute term of 8 x the largest gap between the restatement in fp32 and in fp64, computed in the test from the same
case and the same sequence of steps -- AdaGrad's n needs it too (fp32 alone sits 1.6e-5 relative from fp64 on such rows; times 8 that is
beyond a bare 1e-4).  FTRL's zero pattern: theta == 0 where the fp64 restatement has it, except within 1e-4 (1 + l1) of the threshold,
where at most max(2, 0.1 %) of a table may sit.

Not here: a batch with more segments than one stride of the owner launch covers.  The launch takes its grid from resident_grid with
FMX_GRID_OVER_SGD (fmx_internal.h), whose cap is occupancy x compute units x 65 536 workgroups of four wavefronts -- upwards of 4e9
segments on a device with 256 compute units, beyond the 2^31 entries ensure_segments accepts in a slot -- so the second turn of the
`blk += nwaves * 64` loop cannot be reached through the library; every launch here covered all of its batch's segments in one stride.

Every test prints its own figures (device against the fp64 restatement, the absolute terms in force, the coordinates excluded near
the threshold); the largest ones measured on an MI355X stand in the docstrings of the tests below."""
import numpy as np
import pytest

import datagen
import stateful_cases as SC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL, ASSOC = SC.RTOL, SC.ATOL, SC.ASSOC
PARITY = dict(alpha=0.05, beta=1.0, l1_w=0.5, l1_v=0.3, l2_w=0.01, l2_v=0.01, init_acc=0.0)     # tests/test_ftrl_cpu.py
ADAGRAD = dict(init_acc=1.0, eta=0.05)                                                          # tests/test_gpu_adagrad.py
NAMED = {"adagrad": ADAGRAD, "ftrl": PARITY}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


def _seeds(own):
    """the seeds of a fuzz test: the suite's own, or FMX_FUZZ_SEEDS=lo:hi for a soak run over other seeds (tests/test_gpu_fuzz.py)"""
    import os
    v = os.environ.get("FMX_FUZZ_SEEDS")
    if not v:
        return own
    lo, hi = (int(x) for x in v.split(":"))
    return range(lo, hi)


def read(h, rule, n):
    """(w0, w, v, {table: (linear weights' state, factors' state)}) of the handle, every state row"""
    ids = np.arange(n, dtype=np.uint32)
    if rule == "adagrad":
        nw, nv = h.adapt_state_rows(ids)
        tabs = {"n": (nw, nv)}
    else:
        zw, zv, nw, nv = h.ftrl_state_rows(ids)
        tabs = {"z": (zw, zv), "n": (nw, nv)}
    return h.get_params() + (tabs,)


def same_bits(a, b):
    """two read()s agree bit for bit"""
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
            all(np.array_equal(x, y) for t in a[3] for x, y in zip(a[3][t], b[3][t])))


def compare(got, rule, m, st, st_low, what):
    """the device's parameters, every state row and (FTRL) the zero pattern against the fp64 restatement (m, st); st_low is the fp32
    restatement's state at the same point: 8 x its gap to st is the absolute term of a state table"""
    w0, w, v, dev = got
    ref = SC.tables(rule, st)
    terms = {t: ASSOC * g for t, g in SC.state_gaps(rule, st, st_low).items()}
    print("gaps %s: v %.3g  w %.3g  w0 %.3g  %s" % (rule, SC.gap(v, m.v), SC.gap(w, m.w), abs(w0 - m.w0), "  ".join(
        "%s_v %.3g %s_w %.3g (absolute term %.3g, largest |%s| %.3g)" % (
            t, SC.gap(dev[t][1], ref[t][1]), t, SC.gap(dev[t][0], ref[t][0]), terms[t], t,
            max(float(np.abs(x).max()) if x.size else 0.0 for x in ref[t])) for t in ref)))
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL, err_msg=what)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL, what
    for t in ref:
        np.testing.assert_allclose(dev[t][1], ref[t][1], rtol=RTOL, atol=terms[t], err_msg=what + ": " + t + "_v")
        np.testing.assert_allclose(dev[t][0], ref[t][0], rtol=RTOL, atol=terms[t], err_msg=what + ": " + t + "_w")
    if rule == "ftrl":
        for name, theta64, z64, l1 in SC.zero_tables(m, st):
            SC.check_zero_pattern(name, v if name == "v" else w, theta64, z64, l1, what)


class Twin:
    """one handle and the restatement in fp64 and in fp32, driven through the same steps"""

    def __init__(self, capi, rule, m, task, lr, lo=-1.0, hi=1.0):
        self.capi, self.rule, self.task, self.lr, self.lo, self.hi = capi, rule, task, lr, lo, hi
        self.m64, self.m32 = m.copy(), m.copy()
        self.s64 = self.s32 = self.opts = None
        self.data = {}
        self.h = capi.Handle(m.n, m.k, m.k0, m.k1, task, m.reg0, m.regw, m.regv, lr, lo, hi)
        self.h.set_params(m.w0, m.w, m.v)

    def close(self):
        self.h.close()

    def upload(self, slot, d):
        self.data[slot] = d
        self.h.upload_rows(slot, d.entries, d.row_ptr, d.target)

    def begin(self, opts, restate=True):
        """opens or resets the session; the restatement's state starts from ITS model of this moment"""
        self.opts = dict(opts)
        if self.rule == "adagrad":
            self.h.adapt_begin("adagrad", opts["init_acc"], opts["eta"])
        else:
            self.h.ftrl_begin(**opts)
        if restate:
            self.s64, self.s32 = SC.new_state(self.rule, self.m64, opts), SC.new_state(self.rule, self.m32, opts)

    def epoch(self, slot, batch, chunk, restate=True):
        es = (self.h.adapt_epoch if self.rule == "adagrad" else self.h.ftrl_epoch)(slot, batch, chunk)
        if restate:
            b = int(es.batch_used) if batch == 0 else batch       # batch 0: the library's choice goes to the restatement
            for m, st, dt in ((self.m64, self.s64, np.float64), (self.m32, self.s32, np.float32)):
                SC.rule_epoch(self.rule, m, self.data[slot], self.task, self.lr, self.lo, self.hi, b, chunk, st, self.opts, dtype=dt)
        return es

    def plain_epoch(self, slot, batch, chunk):
        """fmx_sgd_epoch inside the session: the plain batch rule moves the parameters, the state stays"""
        from libfm_amd import adaptive
        self.h.sgd_epoch(slot, self.capi.SGD_MINIBATCH, self.capi.APPLY_SEGMENTED, batch, chunk)
        for m, dt in ((self.m64, np.float64), (self.m32, np.float32)):
            adaptive.epoch(m, self.data[slot], self.task, self.lr, self.lo, self.hi, batch, chunk, None, rule="sgd", dtype=dt)

    def move(self, scale, w_every, v_every):
        """fmx_set_params under the live session: every parameter times `scale`, every w_every-th weight and v_every-th factor row 0 --
        the device's own values on the device, each restatement's own values there; the state is nobody's business"""
        w0, w, v = self.h.get_params()
        for m in (None, self.m64, self.m32):
            p0, pw, pv = (w0, w, v) if m is None else (m.w0, m.w, m.v)
            p0, pw, pv = p0 * scale, pw * scale, pv * scale
            pw[::w_every] = 0.0
            pv[:, ::v_every] = 0.0
            if m is None:
                self.h.set_params(p0, pw, pv)
            else:
                m.w0, m.w[:], m.v[:] = p0, pw, pv

    def check(self, what):
        compare(read(self.h, self.rule, self.m64.n), self.rule, self.m64, self.s64, self.s32, what)


# ---------------------------------------------------------------------------------------------
# seeded random shapes
# ---------------------------------------------------------------------------------------------
def run_case(capi, rule, c):
    """the case's EPOCHS epochs on a fresh handle: (read() after the session began, read() at the end, the epochs' stats)"""
    t = Twin(capi, rule, SC.start_model(c), c.task, SC.LR, c.lo, c.hi)
    try:
        t.upload(0, c.data)
        t.begin(c.opts(rule), restate=False)
        start = read(t.h, rule, c.n)
        stats = [t.epoch(0, c.batch, c.chunk, restate=False) for _ in range(SC.EPOCHS)]
        return start, read(t.h, rule, c.n), stats
    finally:
        t.close()


@pytest.mark.parametrize("rule, seed", [("adagrad", s) for s in _seeds(SC.ADAGRAD_SEEDS)] + [("ftrl", s) for s in _seeds(SC.FTRL_SEEDS)])
def test_random_shape(capi, rule, seed):
    """two epochs of the seed's case: parameters, every state row and the zero pattern against the fp64 restatement; features no row
    touches keep theta and state bit for bit (with k1 off: every linear weight and its state); the stats carry the case's rows, batches,
    batch and micro-chunk; on the first four seeds of each list a second run is bit-identical.

    Measured on an MI355X, largest over the 16 seeds of each optimiser.  AdaGrad: parameters 9.9e-7 (v), 1.6e-7 (w), 2.9e-7 (w0); n 6.1e-2 where
    the largest n is 1.8e5 (absolute terms in force 1.2e-6 .. 6.7e-1).  FTRL: parameters 1.1e-6 (v), 4.3e-7 (w), 9.1e-8 (w0); z 2.5e-4 where the
    largest |z| is 463 (terms 2.9e-6 .. 2.8e-3); n 3.2e-2 where the largest n is 4.4e4 (terms 9.2e-7 .. 1.6e-1); excluded near the threshold at
    most 118 of 527 360 factors (cap 527); no mismatch of the zero pattern."""
    own = seed in (SC.ADAGRAD_SEEDS if rule == "adagrad" else SC.FTRL_SEEDS)
    c, (m64, s64), (_, s32) = SC.restated(rule, seed)
    what = c.describe(rule)
    print(what)
    cond = SC.conditioning(rule, seed)
    if not cond["ok"]:
        assert not own, what + ": a case of the suite's own seeds must be well-conditioned (" + "; ".join(cond["why"]) + ")"
        pytest.skip("ill-conditioned case of a soak run: " + "; ".join(cond["why"]))
    start, end, stats = run_case(capi, rule, c)
    compare(end, rule, m64, s64, s32, what)
    rows = len(c.y)
    for es in stats:
        assert (es.rows, es.batches, es.batch_used, es.w0_chunk_used) == (rows, (rows + c.batch - 1) // c.batch, c.batch, c.chunk), what
    touched = np.zeros(c.n, dtype=bool)
    touched[c.entries["id"]] = True
    idle = ~touched
    assert np.array_equal(end[1][idle], start[1][idle]) and np.array_equal(end[2][:, idle], start[2][:, idle]), what
    for t in end[3]:
        assert np.array_equal(end[3][t][0][idle], start[3][t][0][idle]) and np.array_equal(end[3][t][1][:, idle], start[3][t][1][:, idle]), what
        if not c.k1:
            assert np.array_equal(end[3][t][0], start[3][t][0]), what
    if not c.k1:
        assert np.array_equal(end[1], start[1]), what
    if not c.k0:
        assert end[0] == 0.0, what
    if c.k and touched.any():
        assert (end[2][:, touched] != start[2][:, touched]).any(), what
    if seed in (SC.ADAGRAD_SEEDS[:4] if rule == "adagrad" else SC.FTRL_SEEDS[:4]):
        start2, end2, _ = run_case(capi, rule, c)
        assert same_bits(start, start2) and same_bits(end, end2), what + ": a second identical run differs"


# ---------------------------------------------------------------------------------------------
# named edges of the owner block
# ---------------------------------------------------------------------------------------------
SMALL_N, SMALL_ROWS, SMALL_NNZ = 640, 96, 8
LR = 0.01


def small_model(k, n=SMALL_N, k0=True, k1=True):
    """the parity shape's start values (tests/test_gpu_adagrad.py start_model) at any width, 0 included"""
    m = O.Model(n, k, k0, k1, 0.01, 0.002, 0.001)
    m.v[:] = O.init_values(1, n, max(k, 1), 0.05)[:k]
    if k1:
        m.w[:] = O.init_values(2, n, 1, 0.02)[0]
    m.w0 = 0.03 if k0 else 0.0
    return m


def run_small(capi, rule, k, task, epochs=3):
    t = Twin(capi, rule, small_model(k), task, LR)
    try:
        t.upload(0, O.synth_rows(7, 0, SMALL_ROWS, SMALL_NNZ, SMALL_N))
        t.begin(NAMED[rule])
        for _ in range(epochs):
            es = t.epoch(0, 32, 8)
        assert (es.rows, es.batches, es.batch_used, es.w0_chunk_used) == (SMALL_ROWS, 3, 32, 8)
        t.check("%s k=%d task=%d" % (rule, k, task))
        if k:
            assert SC.gap(t.m64.v, small_model(k).v) > 1e-3        # (the epochs moved the parameters far beyond the tolerances)
        return read(t.h, rule, SMALL_N)
    finally:
        t.close()


@pytest.mark.parametrize("rule", SC.RULES)
@pytest.mark.parametrize("k", [0, 3, 17, 33, 65, 129, 257, 513])
def test_widths_off_the_padding(capi, rule, k):
    """the parity shape cut down (640 features, 96 rows of 8, batch 32, micro-chunk 8) at widths that are not their own padding: no
    factors at all (k 0), a row shorter than KP below 32 (k 3 under KP 4), and the row stride 16 ceil(k / 16) the state tables inherit
    from V under every KP from 32 to 1024 (k 17: 32 floats, 33: 48 under KP 64, 65: 80 under 128, 129: 144 under 256, 257: 272 under 512,
    513: 528 under 1024).

    Measured on an MI355X, largest over the widths.  AdaGrad: parameters 2.7e-8, n 2.3e-6 (absolute terms 3.5e-6 .. 1.1e-5).  FTRL: parameters
    5.6e-8, z 2.3e-6 (terms 6.6e-6 .. 1.9e-5), n 1.7e-6 (terms 3.0e-6 .. 1.9e-5); excluded near the threshold at most 24 of 328 320 factors; no
    mismatch of the zero pattern."""
    run_small(capi, rule, k, k % 2)


@pytest.mark.parametrize("rule", SC.RULES)
@pytest.mark.parametrize("k", [33, 100])
def test_rows_padded_to_kp(capi, rule, k, monkeypatch):
    """FMX_ROW_STRIDE_KP=1 (read by fmx_create): rows of KP floats instead of 16 ceil(k / 16) -- the same numbers bit for bit, since
    the padding holds zeros that no step moves"""
    short = run_small(capi, rule, k, 1)
    monkeypatch.setenv("FMX_ROW_STRIDE_KP", "1")
    padded = run_small(capi, rule, k, 1)
    assert same_bits(short, padded)


SEGMENT_N = 4 * 129 + 7


def segment_rows(S, hot_last, rows=11, seed=0):
    """`rows` rows that touch exactly S distinct features: every feature once, except one (the smallest or the largest id: the first or
    the last segment of the batch) that occurs in every row -- a tail walk of rows - 1 occurrences, and the last segment's end taken
    from batch_nnz"""
    rng = np.random.default_rng(1000 * S + seed)
    ids = np.sort(rng.choice(SEGMENT_N, S, replace=False))
    hot = int(ids[-1] if hot_last else ids[0])
    out = [[] for _ in range(rows)]
    for i, j in enumerate(int(j) for j in ids if j != hot):
        out[i % rows].append(j)
    for r in out:
        r.insert(int(rng.integers(0, len(r) + 1)), hot)

    def val():
        x = round(float(rng.uniform(-1.5, 1.5)), 3)
        return x if x != 0.0 else 0.5
    data = O.Data.from_rows([[(j, val()) for j in r] for r in out], np.round(rng.normal(0, 1, rows), 3).astype(np.float32))
    assert len(set(data.entries["id"].tolist())) == S and len(data.entries) == S - 1 + rows
    return data


SEGMENT_COUNTS = [(k, S) for k in (8, 16, 128, 1024) for S in (1, 2, 63, 64, 65, 127, 128, 129)] + [(16, 33)]


@pytest.mark.parametrize("rule", SC.RULES)
@pytest.mark.parametrize("k, S", SEGMENT_COUNTS)
def test_segment_counts_of_one_batch(capi, rule, k, S):
    """one batch of S segments around every boundary of the round structure (EPI U segment groups a round, 64 segments a wavefront):
    k 8 -- EPI 8, 64 segments a round; k 16 -- EPI 4, U 8, so S = 33 leaves one segment for a second round and S = 65 one for a second
    wavefront; k 128 -- EPI 1, U 4, the last round holds S mod 4 segments; k 1024 -- U 2 for AdaGrad, 1 for FTRL.  The feature that
    occurs in every row is the batch's first segment, then (new rows, same session) its last.

    Measured on an MI355X, largest over the cases.  AdaGrad: parameters 5.9e-7, n 2.0e-4 where the largest n is 99 (absolute terms 2.3e-6 ..
    4.3e-4).  FTRL: parameters 2.1e-7, z 8.7e-6 (terms 1.4e-6 .. 4.3e-5), n 2.6e-5 (terms 1.4e-7 .. 2.0e-4); excluded near the threshold at most
    44 of 535 552 factors; no mismatch of the zero pattern."""
    t = Twin(capi, rule, small_model(k, SEGMENT_N), 0, LR, -2.0, 2.0)
    try:
        t.begin(NAMED[rule])
        for hot_last in (False, True):
            t.upload(0, segment_rows(S, hot_last))
            for _ in range(2):
                es = t.epoch(0, 16, 4)                            # (16 > the slot's 11 rows: one batch)
                assert (es.rows, es.batches, es.batch_used, es.max_feature_count) == (11, 1, 16, 11)
            t.check("%s k=%d S=%d hot_last=%d" % (rule, k, S, hot_last))
    finally:
        t.close()


@pytest.mark.parametrize("rule", SC.RULES)
def test_a_batch_of_empty_rows(capi, rule):
    """three rows without an entry: no segment, so the owner launch is skipped; the bias still moves, nothing else does"""
    k = 8
    m = small_model(k)
    d = O.Data(np.zeros(0, dtype=datagen.ENTRY_DTYPE), np.zeros(4, dtype=np.uint64), np.array([0.7, -0.4, 0.2], dtype=np.float32))
    t = Twin(capi, rule, m, 0, LR)
    try:
        t.upload(0, d)
        t.begin(NAMED[rule])
        start = read(t.h, rule, m.n)
        for _ in range(2):
            es = t.epoch(0, 8, 2)
            assert (es.rows, es.batches, es.max_feature_count) == (3, 1, 0)
        end = read(t.h, rule, m.n)
        t.check(rule + ": empty rows")
        assert abs(end[0] - start[0]) > 1e-3 and same_bits((0.0,) + start[1:], (0.0,) + end[1:])
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
# session orders
# ---------------------------------------------------------------------------------------------
SECOND = {"adagrad": dict(init_acc=0.25, eta=0.2), "ftrl": dict(alpha=0.2, beta=0.5, l1_w=0.05, l1_v=0.05, l2_w=0.0, l2_v=0.01, init_acc=0.25)}


@pytest.mark.parametrize("rule", SC.RULES)
@pytest.mark.parametrize("k", [8, 100])
def test_session_orders(capi, rule, k):
    """one session through what a caller may do between epochs, the restatement driven through the same sequence and everything compared
    after each step: the batch changes 32 -> 50 -> the library's choice -> 32 (the segments are re-bucketed under a live state); two
    slots with different rows alternate; fmx_set_params moves the parameters under the state (times 1.5, some set to 0: FTRL READS theta,
    it does not reconstruct it from z and n); an fmx_sgd_epoch between two stateful epochs leaves the state alone; *_begin again, with
    other options, resets it (FTRL: z from the parameters of that moment).

    Measured on an MI355X, largest over the steps.  AdaGrad: parameters 8.6e-8, n 1.5e-6 (absolute terms 0 right after a begin, else up to
    1.1e-5).  FTRL: parameters 8.1e-8, z 3.4e-6 (terms 1.9e-6 .. 2.9e-5), n 1.5e-6 (terms 0 right after a begin, else up to 1.1e-5); excluded
    near the threshold at most 18 of 64 000 factors; no mismatch of the zero pattern."""
    task = 1
    t = Twin(capi, rule, small_model(k), task, LR)
    step = [0]

    def check(text):
        step[0] += 1
        t.check("%s k=%d step %d (%s)" % (rule, k, step[0], text))
    try:
        t.upload(0, O.synth_rows(7, 0, SMALL_ROWS, SMALL_NNZ, SMALL_N))
        t.upload(1, O.synth_rows(11, 0, 80, 12, SMALL_N))
        t.begin(NAMED[rule])
        for batch in (32, 50, 0, 32):
            es = t.epoch(0, batch, 8)
            assert es.rows == SMALL_ROWS and es.w0_chunk_used == 8 and (es.batch_used == batch if batch else es.batch_used >= 32)
            assert es.batches == (SMALL_ROWS + es.batch_used - 1) // es.batch_used
            check("batch %d" % batch)
        for slot in (1, 0, 1):
            es = t.epoch(slot, 32, 8)
            assert es.rows == (80 if slot else SMALL_ROWS)
            check("slot %d" % slot)
        before = read(t.h, rule, SMALL_N)
        t.move(1.5, 7, 5)
        moved = read(t.h, rule, SMALL_N)
        assert same_bits((0.0, moved[1], moved[2], before[3]), (0.0,) + moved[1:])      # (the state did not move with the parameters)
        assert np.all(moved[1][::7] == 0.0) and np.all(moved[2][:, ::5] == 0.0) and SC.gap(moved[2], before[2]) > 1e-2
        t.epoch(0, 32, 8)
        check("after fmx_set_params")
        t.plain_epoch(1, 32, 8)
        check("after fmx_sgd_epoch")
        t.epoch(1, 32, 8)
        check("the epoch after fmx_sgd_epoch")
        t.begin(SECOND[rule])
        check("begin again")
        t.epoch(0, 50, 3)
        check("the epoch after begin again")
    finally:
        t.close()
