"""CPU: the restated dispatch of FMX_SGD_SEQUENTIAL (tests/seq_routes.py) and the reach of tests/test_gpu_sequential.py.

The GPU tests assert the form each epoch reports against expected_route(); this file checks that the cut they rely on is the greedy cut
of ensure_runs (against a direct row-by-row restatement), and that their cases, by expected_route, reach every kernel instance the mode
can launch.  A form added to the dispatch without a case fails here."""
import numpy as np
import pytest

from common import Golden
import seq_routes as R
import test_gpu_sequential as G


def cut_direct(entries, row_ptr):
    """the cut as a sentence: walk the rows keeping the set of ids the open run holds; a row that repeats an id is a run of its own, a row
    that meets the set, or the 4097th row, opens a new run"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    runs, start, held = [], 0, set()
    for r in range(len(rp) - 1):
        ids = [int(i) for i in entries["id"][rp[r]:rp[r + 1]]]
        if len(set(ids)) < len(ids):
            if r > start:
                runs.append((start, r - start, False))
            runs.append((r, 1, True))
            start, held = r + 1, set()
            continue
        if r > start and (held.intersection(ids) or r - start >= R.RUN_MAX):
            runs.append((start, r - start, False))
            start, held = r, set()
        held.update(ids)
    if start < len(rp) - 1:
        runs.append((start, len(rp) - 1 - start, False))
    return runs


@pytest.mark.parametrize("seed", range(6))
def test_cut_runs_matches_the_direct_cut(seed):
    rng = np.random.default_rng(seed)
    rows = int(rng.integers(200, 3000))
    ent, rp, _, _, _, _ = G.make_rows(seed, rows, int(rng.integers(1, 30)), int(rng.integers(1, 400)), fixed=bool(seed % 2),
                                      dups=int(rng.integers(0, 20)))
    assert R.cut_runs(ent, rp) == cut_direct(ent, rp)


def test_cut_runs_bound_and_empty_rows():
    # 9000 rows that share nothing (every third empty): runs of exactly 4096, 4096, 808
    rows = 9000
    sizes = np.where(np.arange(rows) % 3 == 0, 0, 2)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=G.ENTRY)
    ent["id"] = np.arange(len(ent))
    assert [nb for _, nb, _ in R.cut_runs(ent, rp)] == [4096, 4096, 808]
    assert R.cut_runs(ent, rp) == cut_direct(ent, rp)
    # no entries at all: only the bound cuts
    rp0 = np.zeros(rows + 1, dtype=np.uint64)
    assert [nb for _, nb, _ in R.cut_runs(ent[:0], rp0)] == [4096, 4096, 808]


def test_cut_runs_around_a_repeating_row():
    # rows 0-2 disjoint, row 3 repeats an id, row 4 shares an id with row 3 only, row 5 shares with row 0
    rows = [[1, 2], [3], [4, 5], [6, 6], [6, 7], [1]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    ent = np.zeros(int(rp[-1]), dtype=G.ENTRY)
    ent["id"] = [i for r in rows for i in r]
    # row 4 meets row 3, but row 3 is closed already: 4 opens a run that row 5 extends (row 0 is in an earlier run)
    assert R.cut_runs(ent, rp) == [(0, 3, False), (3, 1, True), (4, 2, False)] == cut_direct(ent, rp)


@pytest.mark.parametrize("s", range(len(G.EDGE_SLOTS)))
@pytest.mark.parametrize("edge", G.EDGE_CASES, ids=str)
def test_edge_slots_cut_exactly(edge, s):
    k, _, _, task, lo, hi = edge
    ent, rp, _, _ = G.edge_rows(G.EDGE_SLOTS[s], lo, hi, seed=31 * k + s)
    runs = R.cut_runs(ent, rp)
    assert [nb for _, nb, _ in runs] == G.split_4096(G.EDGE_SLOTS[s])
    bits, _, n_runs = R.expected_route(k, 1, 1, task, hi, runs)
    assert bits & R.STAT_SEQ_RUNS and n_runs == len(runs)


def _routes():
    """(case name, bits, instances) of every epoch the GPU file runs"""
    out = []
    for name in G.FIXTURES:
        g = Golden(name)
        ent, rp = g.z["train_entries"], g.z["train_row_ptr"]
        runs = R.cut_runs(ent, rp)
        max_row = int(np.diff(rp.astype(np.int64)).max())
        for knobs in G.FORMS:
            bits, inst, _ = R.expected_route(g.k, g.k0, g.k1, g.task, max_row, runs, knobs)
            out.append(("%s[%s]" % (name, G.form_id(knobs)), bits, inst))
    for c in G.online_cases():
        ent, rp, _, _, _, _ = G.case_rows(c)
        max_row = int(np.diff(rp.astype(np.int64)).max())
        bits, inst, _ = R.expected_route(c["k"], c["k0"], c["k1"], c["task"], max_row, R.cut_runs(ent, rp), c["knobs"])
        out.append((c["name"], bits, inst))
    for k, k0, k1, task, lo, hi in G.EDGE_CASES:
        for s, lengths in enumerate(G.EDGE_SLOTS):
            ent, rp, _, _ = G.edge_rows(lengths, lo, hi, seed=31 * k + s)
            bits, inst, _ = R.expected_route(k, k0, k1, task, int(np.diff(rp.astype(np.int64)).max()), R.cut_runs(ent, rp))
            out.append(("edge_k%d_%d" % (k, s), bits, inst))
    return out


@pytest.fixture(scope="module")
def routes():
    return _routes()


def test_cases_reach_every_kernel_instance(routes):
    reached = set().union(*(inst for _, _, inst in routes))
    need = set()
    for task in (0, 1):
        for kp in (8, 16, 32):
            need.add("k_run_fused<%d,%d,%d>" % (kp, kp, task))
        for kp in (64, 128):
            for zr in (16, 40, 64):
                need.add("k_run_fused<%d,%d,%d>" % (kp, zr, task))
    assert len(need) == 18
    for kp in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):          # k_run_apply at every row width, in either task
        assert {"k_run_apply<%d,0>" % kp, "k_run_apply<%d,1>" % kp} & reached, kp
    need |= {"k_apply<%d>" % kp for kp in (4, 8, 128, 512)}                         # the three-launch form at several row widths
    need |= {"k_sequential_wg<64>", "k_sequential_wg<128>", "seq_row_entries<64>", "seq_row_entries<128>"}
    need |= {"k_sequential_rows<64,32>", "k_sequential_rows<64,64>", "k_sequential_rows<128,32>", "k_sequential_rows<128,64>"}
    need |= {"k_sequential<%d>" % kp for kp in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)}
    missing = sorted(need - reached)
    assert not missing, missing
    # both tasks through the two-launch form, the three-launch form and the entry-by-entry loop
    for task in (0, 1):
        assert any(i.startswith("k_run_apply<") and i.endswith(",%d>" % task) for i in reached)


def test_cases_reach_every_status_bit(routes):
    bits = 0
    for _, b, _ in routes:
        bits |= b
    assert bits == R.SEQ_MASK
    # runs and one example at a time both by default (no switch) as well as forced
    names = {n for n, b, _ in routes if b & R.STAT_SEQ_RUNS}
    assert any(n.startswith("runs_") for n in names) and any(n.startswith("seq_") for n in {n for n, _, _ in routes} - names)


def test_every_k_bias_and_linear_term_in_runs_and_out(routes):
    cases = {c["name"]: c for c in G.online_cases()}
    by_name = {n: b for n, b, _ in routes}
    runs_k, seq_k, combos_runs, combos_seq = set(), set(), set(), set()
    for n, c in cases.items():
        if by_name[n] & R.STAT_SEQ_RUNS:
            runs_k.add(c["k"])
            combos_runs.add((c["k0"], c["k1"], c["task"]))
        else:
            seq_k.add(c["k"])
            combos_seq.add((c["k0"], c["k1"], c["task"]))
    assert set(G.KS) <= runs_k and set(G.KS) <= seq_k
    all_combos = {(a, b, t) for a in (0, 1) for b in (0, 1) for t in (0, 1)}
    assert combos_runs == all_combos and combos_seq == all_combos
    # the bias-free branches of the runs kernels (k_run_apply, k_run_fused, k_apply) and the entry-by-entry loop inside runs
    for prefix in ("k_run_apply<", "k_run_fused<", "k_apply<"):
        for k0 in (0, 1):
            assert any(cases[n]["k0"] == k0 and any(i.startswith(prefix) for i in inst) for n, _, inst in routes if n in cases), (prefix, k0)
    assert any(b & R.STAT_SEQ_RUNS and b & R.STAT_SEQ_ENTRIES for _, b, _ in routes)


def test_online_cases_cover_the_row_shapes():
    cases = G.online_cases()
    assert {16, 17, 40, 41, 64, 65, 150, 1000} <= {c["max_row"] for c in cases}
    assert any(c["fixed"] for c in cases) and any(not c["fixed"] for c in cases)
    assert any(c["dups"] for c in cases) and any(c["big"] for c in cases) and any(c["clamp"] for c in cases)
    for c in cases:
        ent, rp, y, n, lo, hi = G.case_rows(c)
        assert int(ent["id"].max(initial=0)) < n and len(rp) == c["rows"] + 1 and len(rp) - 1 <= 10_000
        sizes = np.diff(rp.astype(np.int64))
        assert sizes.max() == c["max_row"]
        if c["fixed"]:
            assert sizes.min() == c["max_row"]
        else:
            assert (sizes == 0).any()
        if c["clamp"]:
            assert (y < lo).any() and (y > hi).any()


def test_determinism_cases_cover_every_form():
    cases = {c["name"]: c for c in G.online_cases()}
    bits = 0
    for name, knobs in G.DET_CASES:
        c = cases[name]
        ent, rp, _, _, _, _ = G.case_rows(c)
        b, _, _ = R.expected_route(c["k"], c["k0"], c["k1"], c["task"], int(np.diff(rp.astype(np.int64)).max()), R.cut_runs(ent, rp), knobs)
        bits |= b
    assert bits == R.SEQ_MASK


def test_forced_runs_on_the_fixtures():
    """FMX_SEQ_RUNS=1 sends the fixtures through the runs kernels the issue names: zipf_k32 through k_run_fused<32,32,1>, ragged_nolin
    (no bias, no linear term) through a bias-free runs kernel"""
    def route(name, knobs):
        g = Golden(name)
        rp = g.z["train_row_ptr"]
        return g, R.expected_route(g.k, g.k0, g.k1, g.task, int(np.diff(rp.astype(np.int64)).max()), R.cut_runs(g.z["train_entries"], rp), knobs)
    g, (bits, inst, _) = route("sgd_cls_zipf_k32", {"FMX_SEQ_RUNS": "1"})
    assert "k_run_fused<32,32,1>" in inst
    g, (bits, inst, _) = route("sgd_reg_ragged_nolin", {"FMX_SEQ_RUNS": "1"})
    assert g.k0 == 0 and g.k1 == 0 and bits & R.STAT_SEQ_RUNS and inst & {i for i in inst if i.startswith("k_run_")}
    for name in G.FIXTURES:                                       # by default every fixture runs one example at a time
        _, (bits, _, _) = route(name, {})
        assert not bits & R.STAT_SEQ_RUNS
