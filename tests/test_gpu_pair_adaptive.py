"""GPU: pairwise ranking (BPR) on the batch rule stepped by an open session's per-coordinate rule -- fmx_adapt_pair_epoch[_sampled],
fmx_ftrl_pair_epoch[_sampled], k_pair_apply_rule -- against the float64 restatements libfm_amd/adaptive.py pair_epoch and
libfm_amd/ftrl.py pair_epoch (themselves pinned in tests/test_pair_adaptive_cpu.py), after 3 epochs with AdaGrad (eta 0.05, init_acc 1)
and FTRL (alpha 0.05, beta 1, l1 (2.0, 1.0), l2 (0.01, 0.02), init_acc 0).

Tolerances, the project's for stateful rules.  Parameters rtol 1e-4 / atol 2e-5; AdaGrad's n rtol 1e-4; w0 as tests/test_gpu_bpr.py;
FTRL's z and n rtol 1e-4 plus 8 x the gap between the restatement with the float32 step and with the float64 step at the test's own
shape, computed in the test (tests/test_gpu_ftrl.py's method and factor); the zero pattern as its check_zero_pattern.  Every test
prints its gaps."""
import contextlib
import io

import numpy as np
import pytest

import bpr_sampled_oracle as S
import datagen
import pair_adaptive_cases as PC
from test_gpu_bpr import handle, rows_and_pairs, w0_close
from test_gpu_bpr_sampled import exclusion_lists, two_slots, upload
from test_gpu_ftrl import check_zero_pattern

pytestmark = pytest.mark.gpu

RTOL, ATOL, ASSOC = 1e-4, 2e-5, 8.0
RULES = ["adagrad", "ftrl"]


def begin(h, rule, opts=None):
    if rule == "adagrad":
        o = opts or PC.ADA
        h.adapt_begin("adagrad", o["init_acc"], o["eta"])
    else:
        h.ftrl_begin(**(opts or PC.FTRL))


def dev_state(h, rule, n):
    ids = np.arange(n, dtype=np.uint32)
    return h.adapt_state_rows(ids) if rule == "adagrad" else h.ftrl_state_rows(ids)


def reference(rule, m0, epochs_pairs, batch, opts=None):
    """(fp64 restatement model, state, absolute terms (z, n) of FTRL's state)"""
    if rule == "adagrad":
        return PC.restate(rule, m0, epochs_pairs, batch, opts=opts) + ((0.0, 0.0),)
    _, g, (m, st), _ = PC.step_gaps(rule, m0, epochs_pairs, batch, opts)
    return m, st, (ASSOC * max(g[0], g[1]), ASSOC * max(g[2], g[3]))


def check(h, rule, m, st, terms, what, opts=None):
    w0, w, v = h.get_params()
    dev = dev_state(h, rule, m.n)
    ref = PC.state_arrays(rule, st)
    print("%s %s gaps: v %.3g  w %.3g  w0 %.3g  state %s  (absolute terms: z %.3g  n %.3g)" % (
        what, rule, PC.gap(v, m.v), PC.gap(w, m.w), abs(w0 - m.w0), ["%.3g" % PC.gap(a, b) for a, b in zip(dev, ref)], terms[0], terms[1]))
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    w0_close(w0, m.w0)
    if rule == "adagrad":
        for a, b in zip(dev, ref):
            np.testing.assert_allclose(a, b, rtol=RTOL)
    else:
        for a, b, t in zip(dev, ref, (terms[0], terms[0], terms[1], terms[1])):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=t)
        o = opts or PC.FTRL
        check_zero_pattern("v", v, m.v, st.z_v, o["l1_v"])
        if m.k1:
            check_zero_pattern("w", w, m.w, st.z_w, o["l1_w"])
    return w, v


def stored(rule, ent, rp, pa, pb, k, batch, n, m0, epochs=3):
    """`epochs` epochs over stored pairs on the device from m0; returns the handle (its session open)"""
    from libfm_amd import capi
    h = handle(capi, n, k, m0.k0, m0.k1, (m0.reg0, m0.regw, m0.regv), 0.05, m0)
    h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
    h.upload_pairs(0, pa, pb)
    begin(h, rule)
    for _ in range(epochs):
        st = (h.adapt_pair_epoch if rule == "adagrad" else h.ftrl_pair_epoch)(0, batch)
        assert st.rows == len(pa) and st.batch_used == batch and st.batches == (len(pa) + batch - 1) // batch
        assert st.max_feature_count >= 1 and st.main_kernel_launches == 2 * st.batches and st.device_seconds > 0
    return h


def sampled(rule, d, k, batch, n, m0, n_neg, seed, epochs=3, exclude=True, draws=1):
    from libfm_amd import capi
    h = handle(capi, n, k, m0.k0, m0.k1, (m0.reg0, m0.regw, m0.regv), 0.05, m0)
    upload(h, d, exclude)
    begin(h, rule)
    P = len(d[4]) * n_neg
    for ep in range(epochs):
        st, forced = (h.adapt_pair_epoch_sampled if rule == "adagrad" else h.ftrl_pair_epoch_sampled)(0, batch, n_neg, seed, ep, draws)
        assert forced == 0 and st.rows == P and st.batch_used == batch and st.batches == (P + batch - 1) // batch
        assert st.setup_seconds > 0 and st.device_seconds > 0
    return h


def joined(d, n_neg, seed, epochs, exclude=True):
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    out = []
    for ep in range(epochs):
        ent, rp, pa, pb, _, forced = S.epoch_pairs(q_ent, q_rp, c_ent, c_rp, q, c, n_neg, seed, ep, ex if exclude else None)
        assert forced == 0
        out.append((ent, rp, pa, pb))
    return out


@pytest.mark.parametrize("batch", [1, 7, 64, 600])
@pytest.mark.parametrize("rule", RULES)
def test_stored_pairs_match_the_restatement(rule, batch):
    n, k = 50, 8
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    m0 = PC.start_model(n, k)
    m, st, terms = reference(rule, m0, [(ent, rp, pa, pb)] * 3, batch)
    h = stored(rule, ent, rp, pa, pb, k, batch, n, m0)
    try:
        w, v = check(h, rule, m, st, terms, "stored B %d" % batch)
    finally:
        h.close()
    assert PC.gap(m.v, m0.v) > 1e-3
    if rule == "ftrl":
        assert 0.02 < (v == 0).mean() < 0.5 and 0.02 < (w == 0).mean() < 0.5


@pytest.mark.parametrize("batch", [1, 7, 64, 600])
@pytest.mark.parametrize("rule", RULES)
def test_sampled_pairs_match_the_restatement(rule, batch):
    n, k, n_neg, seed = 50, 8, 2, 23
    d = two_slots(n, 60, 40, 250, 7, 500, empty_every=11)
    m0 = PC.start_model(n, k)
    m, st, terms = reference(rule, m0, joined(d, n_neg, seed, 3), batch)
    h = sampled(rule, d, k, batch, n, m0, n_neg, seed)
    try:
        check(h, rule, m, st, terms, "sampled B %d" % batch)
    finally:
        h.close()


@pytest.mark.parametrize("k", [1, 5, 64, 128, 1000])
@pytest.mark.parametrize("rule", RULES)
def test_widths_with_edge_rows(rule, k):
    """every VEC and a row shorter than KP, B = 7, with test_edge_cases_both_modes' rows: a pair with a == b, empty rows, ids repeated
    inside a row and shared by both rows; then the sampled path (the query's entries once) with test_minibatch_edge_cases' rows"""
    n = 40
    ent, rp, pa, pb = rows_and_pairs(n, 80, 60 if k >= 128 else 200, 8, 61 + k, empty_every=9)
    pa[3] = pb[3] = 5
    pa[4], pb[4] = 8, 17
    pa[5], pb[5] = 8, 2
    m0 = PC.start_model(n, k, seed=k)
    m, st, terms = reference(rule, m0, [(ent, rp, pa, pb)] * 3, 7)
    h = stored(rule, ent, rp, pa, pb, k, 7, n, m0)
    try:
        check(h, rule, m, st, terms, "stored k %d" % k)
    finally:
        h.close()
    d = two_slots(n, 30, 24, 40 if k >= 128 else 120, 6, 600 + k, empty_every=7)
    d[4][3], d[5][3] = 6, 6
    m, st, terms = reference(rule, m0, joined(d, 1, 29, 3, exclude=False), 7)
    h = sampled(rule, d, k, 7, n, m0, 1, 29, exclude=False)
    try:
        check(h, rule, m, st, terms, "sampled k %d" % k)
    finally:
        h.close()


@pytest.mark.parametrize("rule", RULES)
def test_one_feature_in_every_pair_of_a_4096_batch(rule):
    """one segment of 8 192 (stored) / 4 096 (sampled: the query's entry once) entries: the whole batch through one owner"""
    n, k, P = 400, 8, 4096
    rng = np.random.default_rng(71)
    ids = [[0] + rng.integers(1, n, 2).tolist() for _ in range(600)]
    vals = [[1.0] + rng.uniform(-1, 1, 2).round(3).tolist() for _ in range(600)]
    ent, rp, _ = datagen._pack(ids, vals, [0.0] * 600)
    pa, pb = rng.integers(0, 600, P).astype(np.uint32), rng.integers(0, 600, P).astype(np.uint32)
    m0 = PC.start_model(n, k)
    m, st, terms = reference(rule, m0, [(ent, rp, pa, pb)], P)
    h = stored(rule, ent, rp, pa, pb, k, P, n, m0, epochs=1)
    try:
        check(h, rule, m, st, terms, "stored 4096")
        es = (h.adapt_pair_epoch if rule == "adagrad" else h.ftrl_pair_epoch)(0, P)
        assert es.max_feature_count == 2 * P
    finally:
        h.close()
    c_ent, c_rp, _ = datagen._pack([rng.integers(1, n, 2).tolist() for _ in range(200)],
                                   [rng.uniform(-1, 1, 2).round(3).tolist() for _ in range(200)], [0.0] * 200)
    q, c = rng.integers(0, 300, P).astype(np.uint32), rng.integers(0, 200, P).astype(np.uint32)
    d = (ent[:int(rp[300])], rp[:301], c_ent, c_rp, q, c, exclusion_lists(rng, 300, 200))
    m, st, terms = reference(rule, m0, joined(d, 1, 31, 1), P)
    h = sampled(rule, d, k, P, n, m0, 1, 31, epochs=1)
    try:
        check(h, rule, m, st, terms, "sampled 4096")
        es, _ = (h.adapt_pair_epoch_sampled if rule == "adagrad" else h.ftrl_pair_epoch_sampled)(0, P, 1, 31, 1)
        assert es.max_feature_count == P
    finally:
        h.close()


@pytest.mark.parametrize("rule", RULES)
def test_hardest_negatives_equal_the_stored_path_on_the_join(rule):
    """draws = 4: the sampled epoch against the stored-pair epoch on the materialised join of the SAME negatives, both on the device"""
    from libfm_amd import capi
    n, k, n_neg, seed, batch = 300, 64, 2, 41, 64
    d = two_slots(n, 200, 150, 1500, 10, 700, empty_every=13)
    q_ent, q_rp, c_ent, c_rp, q, c, ex = d
    m0 = PC.start_model(n, k)
    new = handle(capi, n, k, True, True, (0.01, 0.01, 0.02), 0.05, m0)
    old = handle(capi, n, k, True, True, (0.01, 0.01, 0.02), 0.05, m0)
    try:
        upload(new, d)
        begin(new, rule)
        begin(old, rule)
        for ep in range(2):
            neg, forced = new.pair_sample(0, n_neg, seed, ep, draws=4)      # (under the parameters the epoch starts from)
            assert forced == 0
            ent, rp, pa, pb = S.join_rows(q_ent, q_rp, c_ent, c_rp, q, c, neg, n_neg)
            old.upload_rows(2, ent, rp, None)
            old.upload_pairs(2, pa, pb)
            (old.adapt_pair_epoch if rule == "adagrad" else old.ftrl_pair_epoch)(2, batch)
            _, f = (new.adapt_pair_epoch_sampled if rule == "adagrad" else new.ftrl_pair_epoch_sampled)(0, batch, n_neg, seed, ep, 4)
            assert f == 0
        (w0o, wo, vo), (w0n, wn, vn) = old.get_params(), new.get_params()
        so, sn = dev_state(old, rule, n), dev_state(new, rule, n)
        print("hardest %s gaps: v %.3g  w %.3g  state %s" % (rule, PC.gap(vn, vo), PC.gap(wn, wo), ["%.3g" % PC.gap(a, b) for a, b in zip(sn, so)]))
        np.testing.assert_allclose(vn, vo, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(wn, wo, rtol=RTOL, atol=ATOL)
        assert abs(w0n - w0o) <= 1e-12 * abs(w0o)
        assert PC.gap(vo, m0.v) > 1e-3
    finally:
        old.close()
        new.close()


@pytest.mark.parametrize("rule", RULES)
def test_bit_reproducible_across_two_handles(rule):
    n, k = 300, 64
    ent, rp, pa, pb = rows_and_pairs(n, 2000, 6000, 12, 41)
    d = two_slots(n, 400, 300, 3000, 12, 800)
    m0 = PC.start_model(n, k)
    res = []
    for _ in range(2):
        h = stored(rule, ent, rp, pa, pb, k, 64, n, m0, epochs=2)
        try:
            upload(h, d, qs=1, cs=2)
            for ep in range(2):
                (h.adapt_pair_epoch_sampled if rule == "adagrad" else h.ftrl_pair_epoch_sampled)(1, 64, 2, 5, ep)
            res.append(h.get_params() + tuple(dev_state(h, rule, n)))
        finally:
            h.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rule", RULES)
def test_pointwise_and_pairwise_epochs_alternate_in_one_session(rule, oracle):
    """fmx_adapt_epoch / fmx_ftrl_epoch and the pairwise epochs step the same tables: pointwise, pairwise, pointwise, pairwise against
    the two restatements sharing one state"""
    from libfm_amd import adaptive, capi, ftrl
    n, k, lr = 50, 8, 0.05
    ent, rp, pa, pb = rows_and_pairs(n, 150, 500, 9, 31)
    y = np.random.default_rng(5).integers(1, 6, len(rp) - 1).astype(np.float32)
    data = oracle.Data(ent, rp, y)
    m0 = PC.start_model(n, k)
    runs = {}
    for dt in ((np.float64, np.float32) if rule == "ftrl" else (np.float64,)):
        m = m0.copy()
        st = PC.make_state(rule, m)
        for _ in range(2):
            if rule == "adagrad":
                adaptive.epoch(m, data, 0, lr, 1.0, 5.0, 64, 16, st, eta=PC.ADA["eta"], dtype=dt)
            else:
                ftrl.epoch(m, data, 0, lr, 1.0, 5.0, 64, 16, st, dtype=dt)
            PC.rule_epoch(rule, m, st, ent, rp, pa, pb, 64, dt)
        runs[dt] = (m, st)
    m, st = runs[np.float64]
    terms = (0.0, 0.0)
    if rule == "ftrl":
        g = [PC.gap(a, b) for a, b in zip(PC.state_arrays(rule, st), PC.state_arrays(rule, runs[np.float32][1]))]
        terms = (ASSOC * max(g[0], g[1]), ASSOC * max(g[2], g[3]))
    h = handle(capi, n, k, True, True, (m0.reg0, m0.regw, m0.regv), lr, m0)
    try:
        h.upload_rows(0, ent, rp, y)
        h.upload_pairs(0, pa, pb)
        begin(h, rule)
        for _ in range(2):
            (h.adapt_epoch if rule == "adagrad" else h.ftrl_epoch)(0, 64, 16)
            (h.adapt_pair_epoch if rule == "adagrad" else h.ftrl_pair_epoch)(0, 64)
        w0, w, v = h.get_params()
        dev, ref = dev_state(h, rule, n), PC.state_arrays(rule, st)
        print("alternating %s gaps: v %.3g  w %.3g  w0 %.3g  state %s" % (rule, PC.gap(v, m.v), PC.gap(w, m.w), abs(w0 - m.w0),
                                                                       ["%.3g" % PC.gap(a, b) for a, b in zip(dev, ref)]))
        np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
        assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + ATOL          # (the pointwise epochs step the bias in fp32 sums: test_gpu_adagrad's bound)
        for i, (a, b) in enumerate(zip(dev, ref)):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=0.0 if rule == "adagrad" else terms[i // 2])
    finally:
        h.close()


def test_refusals_then_a_good_call():
    from libfm_amd import capi
    n, k = 50, 4
    ent, rp, pa, pb = rows_and_pairs(n, 60, 100, 6, 81, dup=False)
    d = two_slots(n, 30, 24, 60, 5, 83)
    m0 = PC.start_model(n, k)
    h = handle(capi, n, k, True, True, (m0.reg0, m0.regw, m0.regv), 0.05, m0)

    def code(fn, *a, **kw):
        with pytest.raises(capi.FmxError) as e:
            fn(*a, **kw)
        return e.value

    calls = {"adagrad": (h.adapt_pair_epoch, h.adapt_pair_epoch_sampled), "ftrl": (h.ftrl_pair_epoch, h.ftrl_pair_epoch_sampled)}
    try:
        h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
        upload(h, d, qs=1, cs=2)
        # without pairs / interactions / a session
        for st_fn, sm_fn in calls.values():
            assert code(st_fn, 0, 16).code == -3                 # no pairs on the slot (the plain call's refusal)
            assert code(sm_fn, 0, 16).code == -3                 # no interactions on the slot
        h.upload_pairs(0, pa, pb)
        for st_fn, sm_fn in calls.values():
            assert code(st_fn, 0, 16).code == -3                 # no session
            assert code(sm_fn, 1, 16).code == -3
        assert h.lib.fmx_adapt_pair_epoch(h.h, 0, None, None) == -1 and h.lib.fmx_ftrl_pair_epoch_sampled(h.h, 1, None, None, None) == -1
        before = h.get_params()
        for rule in RULES:
            begin(h, rule)
            st_fn, sm_fn = calls[rule]
            other_st, other_sm = calls["ftrl" if rule == "adagrad" else "adagrad"]
            assert code(other_st, 0, 16).code == -3              # the other rule's session is open, not this one's
            assert code(other_sm, 1, 16).code == -3
            for mode in (capi.SGD_SEQUENTIAL, capi.SGD_HOGWILD):
                for e in (code(st_fn, 0, 16, mode=mode), code(sm_fn, 1, 16, mode=mode)):
                    assert e.code == -4 and "FMX_SGD_MINIBATCH" in e.text and "batch = 1" in e.text
            assert code(st_fn, 0, 16, mode=7).code == -1         # unknown mode
            assert code(st_fn, 5, 16).code == -3                 # a slot never uploaded
            assert code(sm_fn, 1, 16, n_neg=0).code == -1        # what the plain sampled call refuses
            assert code(sm_fn, 1, 16, draws=17).code == -1
            h.als_begin(0)
            assert code(st_fn, 0, 16).code == -3                 # an open ALS session on the slot
            h.als_end()
            for a, b in zip(before, h.get_params()):
                assert np.array_equal(a, b)                      # (no refusal launched anything)
            es = st_fn(0, 16)                                    # ... and the handle and the session work afterwards
            assert es.rows == len(pa) and es.batches == 7
            es, forced = sm_fn(1, 16, 2, 3, 0)
            assert es.rows == 2 * len(d[4])
            h.pair_epoch(0, capi.SGD_MINIBATCH, 16)              # the plain epoch still runs during a session and leaves the state alone
            s0 = dev_state(h, rule, n)
            h.pair_epoch(0, capi.SGD_SEQUENTIAL)
            for a, b in zip(s0, dev_state(h, rule, n)):
                assert np.array_equal(a, b)
            (h.adapt_end if rule == "adagrad" else h.ftrl_end)()
            h.set_params(m0.w0, m0.w, m0.v)
            before = h.get_params()
    finally:
        h.close()
    s = capi.Handle(n, k, True, True, capi.TASK_REGRESSION, 0.0, 0.01, 0.01, 0.05, 1.0, 5.0, device=0, shard_rank=0, shard_world=2)
    try:
        s.set_params(m0.w0, m0.w, m0.v)
        s.upload_rows(0, ent, rp, None)
        s.upload_pairs(0, pa, pb)
        assert code(s.adapt_pair_epoch, 0, 16).code == -4        # a feature shard: the plain call's refusal
        assert code(s.ftrl_pair_epoch, 0, 16).code == -4
    finally:
        s.close()


def test_adagrad_converges_on_the_device_where_the_plain_rule_diverges():
    """the popularity-skewed case of tests/test_pair_adaptive_cpu.py at B = 2 048 and eta 0.5: the loss of fmx_pair_evaluate falls in
    each of six epochs and no coordinate moves by more than eta in an epoch's one batch"""
    from libfm_amd import capi
    ent, rp, pa, pb, m0 = PC.skewed_case()
    eta = PC.SKEW_ETA
    h = handle(capi, m0.n, m0.k, False, True, (0.0, m0.regw, m0.regv), eta, m0)
    try:
        h.upload_rows(0, ent, rp, np.zeros(len(rp) - 1, np.float32))
        h.upload_pairs(0, pa, pb)
        h.adapt_begin("adagrad", 1.0, eta)
        losses, steps = [h.pair_evaluate(0).loss], []
        _, w, v = h.get_params()
        for _ in range(6):
            es = h.adapt_pair_epoch(0, PC.SKEW_B)
            assert es.batches == 1
            _, w1, v1 = h.get_params()
            steps.append(max(PC.gap(w1, w), PC.gap(v1, v)))
            w, v = w1, v1
            losses.append(h.pair_evaluate(0).loss)
        print("adagrad on the device: loss %s  largest steps %s" % (np.round(losses, 4), np.round(steps, 5)))
        assert all(b < a for a, b in zip(losses, losses[1:]))
        assert max(steps) <= eta * (1.0 + 1e-6)
        h.adapt_end()
        h.set_params(m0.w0, m0.w, m0.v)
        h.pair_epoch(0, capi.SGD_MINIBATCH, PC.SKEW_B)           # (reported: the plain rule at the same batch and rate)
        print("plain rule after one epoch: loss %.4g (start %.4f)" % (h.pair_evaluate(0).loss, losses[0]))
    finally:
        h.close()


def read_model(path, n_attr):
    txt = open(path).read().splitlines()
    assert txt[0] == "#global bias W0" and txt[2] == "#unary interactions Wj"
    w = np.array([float(x) for x in txt[3:3 + n_attr]])
    v = np.array([[float(x) for x in ln.split()] for ln in txt[4 + n_attr:4 + 2 * n_attr]]).T
    return float(txt[1]), w, v


@pytest.mark.parametrize("rule", RULES)
def test_learner_and_cli(rule, oracle, tmp_path, capsys):
    """`-method bpr -optimizer adagrad | ftrl` for four iterations ends at the parameters the restatement, driven the same way, ends at
    (FTRL: and prints the zero counts of the model it saved); FMLearnPairAdaptive driven directly does the same on stored pairs and
    trains on interactions; the CLI runs -interactions through the same learner"""
    from libfm_amd import cli
    from libfm_amd import learner as L
    from libfm_amd import refrand as R
    nu, ni, k, iters, batch = 30, 20, 8, 4, 64
    rng = np.random.default_rng(3)
    f = {x: str(tmp_path / x) for x in ("tr", "te", "trp", "tep", "model", "c", "inter")}
    sets = {}
    for tag, seed, rows in (("tr", 111, 600), ("te", 112, 200)):
        ent, rp, y = datagen.movielens_shaped(nu, ni, rows, seed, noise=0.1)
        oracle.Data(ent, rp, y).write_libsvm(f[tag])
        a, b = rng.integers(0, rows, 400), rng.integers(0, rows, 400)
        keep = y[a] != y[b]
        a, b = a[keep], b[keep]
        hi = y[a] > y[b]
        pa, pb = np.where(hi, a, b).astype(np.uint32), np.where(hi, b, a).astype(np.uint32)
        with open(f[tag + "p"], "w") as fh:
            fh.write("".join("%d %d\n" % (x, z) for x, z in zip(pa, pb)))
        sets[tag] = (ent, rp, y, pa, pb)
    argv = ["-method", "bpr", "-train", f["tr"], "-test", f["te"], "-train_pairs", f["trp"], "-test_pairs", f["tep"], "-dim", "1,1,%d" % k,
            "-iter", str(iters), "-learn_rate", "0.05", "-regular", "0.001,0.01,0.02", "-init_stdev", "0.1", "-seed", "7", "-batch", str(batch),
            "-save_model", f["model"], "-optimizer", rule]
    argv += ["-init_acc", "0.5"] if rule == "adagrad" else ["-ftrl_alpha", "0.1", "-ftrl_beta", "0.5", "-l1", "0.3,0.2"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    err = capsys.readouterr().err
    assert "ERROR" not in err, err
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]
    assert len(lines) == iters and "Final\tTrain=" in buf.getvalue()
    ent, rp, y, pa, pb = sets["tr"]
    n_attr = max(int(ent["id"].max()), int(sets["te"][0]["id"].max())) + 1
    m = oracle.Model(n_attr, k, True, True, 0.001, 0.01, 0.02)
    R.srand(7)
    m.v[:] = R.init_v(k, n_attr, 0.0, 0.1)
    m0 = m.copy()
    opts = dict(eta=0.05, init_acc=0.5) if rule == "adagrad" else dict(alpha=0.1, beta=0.5, l1_w=0.3, l1_v=0.2, l2_w=0.01, l2_v=0.02, init_acc=0.0)
    m, st = PC.restate(rule, m0, [(ent, rp, pa, pb)] * iters, batch, opts=opts)
    w0, w, v = read_model(f["model"], n_attr)
    print("cli %s gaps: v %.3g  w %.3g" % (rule, PC.gap(v, m.v), PC.gap(w, m.w)))
    # (the model file holds 6 significant digits: 5e-7 relative, inside the tolerances)
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=ATOL)
    assert abs(w0 - m.w0) <= 1e-5 * abs(m.w0)
    sp_line = [ln for ln in err.splitlines() if ln.startswith("sparsity\t")]
    if rule == "ftrl":
        check_zero_pattern("v", v, m.v, st.z_v, 0.2)
        check_zero_pattern("w", w, m.w, st.z_w, 0.3)
        got = {a: int(b) for a, b in (t.split("=") for t in sp_line[0].split("\t")[1:])}
        assert len(sp_line) == 1 and got["v_zero"] == int((v == 0).sum()) and got["w_zero"] == int((w == 0).sum()) and got["features"] == n_attr
    else:
        assert not sp_line
    # the learner, driven directly: stored pairs, then interactions on a fresh learner
    def learner():
        fm = L.FMModel()
        fm.num_attribute, fm.num_factor, fm.reg0, fm.regw, fm.regv = n_attr, k, 0.001, 0.01, 0.02
        fm.w0, fm.w, fm.v = 0.0, np.zeros(n_attr), m0.v.copy()
        l = L.FMLearnPairAdaptive()
        l.fm, l.num_iter, l.learn_rate, l.batch, l.optimizer, l.out = fm, iters, 0.05, batch, rule, io.StringIO()
        if rule == "adagrad":
            l.init_acc = 0.5
        else:
            l.ftrl_alpha, l.ftrl_beta, l.l1_w, l.l1_v = 0.1, 0.5, 0.3, 0.2
        l.init()
        return l, fm
    l, fm = learner()
    try:
        te = sets["te"]
        l.learn(L.Data(ent, rp, y), (pa, pb), L.Data(te[0], te[1], te[2]), (te[3], te[4]))
        sp = l.sparsity()
    finally:
        l.close()
    np.testing.assert_allclose(fm.v, m.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(fm.w, m.w, rtol=RTOL, atol=ATOL)
    assert sp.v_zero == int((fm.v == 0).sum()) and len(l.log) == iters
    q_ent, q_rp, q_y = datagen._pack([[u] for u in range(nu)], [[1.0]] * nu, [0.0] * nu)
    c_ent, c_rp, c_y = datagen._pack([[nu + i] for i in range(ni)], [[1.0]] * ni, [0.0] * ni)
    q, c = rng.integers(0, nu, 300).astype(np.uint32), rng.integers(0, ni, 300).astype(np.uint32)
    ref, rst = PC.restate(rule, m0, joined((q_ent, q_rp, c_ent, c_rp, q, c, None), 2, 9, iters, exclude=False), batch, opts=opts)
    l, fm = learner()
    try:
        l.learn_implicit(L.Data(q_ent, q_rp, q_y), L.Data(c_ent, c_rp, c_y), (q, c), None, n_neg=2, seed=9, exclude=None)
    finally:
        l.close()
    print("learn_implicit %s gaps: v %.3g  w %.3g" % (rule, PC.gap(fm.v, ref.v), PC.gap(fm.w, ref.w)))
    np.testing.assert_allclose(fm.v, ref.v, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(fm.w, ref.w, rtol=RTOL, atol=ATOL)
    # the command line with -interactions
    oracle.Data(q_ent, q_rp, q_y).write_libsvm(f["tr"])
    oracle.Data(c_ent, c_rp, c_y).write_libsvm(f["c"])
    with open(f["inter"], "w") as fh:
        fh.write("".join("%d %d\n" % (x, z) for x, z in zip(q, c)))
    argv = ["-method", "bpr", "-train", f["tr"], "-test", f["tr"], "-candidates", f["c"], "-interactions", f["inter"], "-neg", "2",
            "-dim", "1,1,%d" % k, "-iter", "3", "-learn_rate", "0.05", "-seed", "7", "-batch", str(batch), "-optimizer", rule]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    err = capsys.readouterr().err
    assert "ERROR" not in err, err
    assert len([ln for ln in buf.getvalue().splitlines() if ln.startswith("#Iter=")]) == 3 and "Final\tTrain=" in buf.getvalue()
    assert len([ln for ln in err.splitlines() if ln.startswith("sparsity\t")]) == (1 if rule == "ftrl" else 0)
