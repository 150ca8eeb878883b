"""CPU: every seed tests/test_gpu_stateful_fuzz.py runs through the AdaGrad and FTRL kernels is well-conditioned -- the float64
restatement (libfm_amd/adaptive.py, libfm_amd/ftrl.py) of the case's two epochs, with the case's batch, micro-chunk and options, against
the same restatement in fp32.  A failure here says "ill-conditioned case", not "kernel wrong": the seed is replaced in
tests/stateful_cases.py before the device is asked anything about it.

The conditions: the largest fp32-vs-fp64 gap of any parameter <= 2.5e-6 (8 x it, the allowance for the device's other association of the
sums, stays within the project's atol of 2e-5); for FTRL at most max(2, 0.1 %) of a table's coordinates within 1e-4 (1 + l1) of the L1
threshold, and the same zero pattern in fp32 and fp64 on every other coordinate.  Every test prints its figures."""
import numpy as np
import pytest

import stateful_cases as SC


def test_the_generator_reaches_what_it_is_for():
    """over the suite's own seeds: empty rows, repeated ids, batch 1 and a batch larger than the slot, micro-chunk 1 and 300, k = 0, widths
    that are not their own padding, k0 / k1 off, both tasks; and the refused FTRL option set is never drawn"""
    cs = [SC.case(s) for s in SC.ADAGRAD_SEEDS + SC.FTRL_SEEDS]
    sizes = [np.diff(c.row_ptr.astype(np.int64)) for c in cs]
    assert any((z == 0).any() for z in sizes) and any(len(set(z.tolist())) > 1 for z in sizes)
    assert any(any(len(set(c.entries["id"][a:b].tolist())) < b - a for a, b in zip(c.row_ptr[:-1].astype(int), c.row_ptr[1:].astype(int))) for c in cs)
    assert any(c.batch == 1 for c in cs) and any(c.batch > len(c.y) for c in cs) and any(len(c.y) % c.batch for c in cs)
    assert any(c.chunk == 1 for c in cs) and any(c.chunk == 300 for c in cs)
    assert any(c.k == 0 for c in cs) and any(c.k in (3, 5, 13, 17, 31, 33, 65, 100, 129) for c in cs)
    assert any(not c.k0 for c in cs) and any(not c.k1 for c in cs) and {c.task for c in cs} == {0, 1}
    assert all(c.k in SC.WIDTHS and c.batch in SC.BATCHES and c.chunk in SC.CHUNKS and len(c.y) <= 900 for c in cs)
    assert all(not (c.ftrl["beta"] == 0.0 and c.ftrl["init_acc"] == 0.0) for c in cs)
    assert len({tuple(sorted(c.ftrl.items())) for c in cs}) > 8 and len({tuple(sorted(c.adagrad.items())) for c in cs}) > 4


@pytest.mark.parametrize("seed", SC.ADAGRAD_SEEDS)
def test_adagrad_seed_is_well_conditioned(seed):
    c, (m64, s64), _ = SC.restated("adagrad", seed)
    cond = SC.conditioning("adagrad", seed)
    print(c.describe("adagrad"))
    print("fp32 vs fp64: parameters %.3g  n %.3g (relative %.3g; max n %.3g)" % (
        cond["param_gap"], cond["state_gaps"]["n"], cond["n_rel_gap"], max(s64.n_w.max(), s64.n_v.max() if s64.n_v.size else 0.0)))
    assert cond["ok"], "ill-conditioned case (replace the seed): " + "; ".join(cond["why"])
    assert SC.param_gap(m64, SC.start_model(c)) > 1e-4           # (the epochs moved the parameters beyond the tolerances)
    assert np.isfinite(m64.v).all() and np.isfinite(m64.w).all()


@pytest.mark.parametrize("seed", SC.FTRL_SEEDS)
def test_ftrl_seed_is_well_conditioned(seed):
    c, (m64, s64), _ = SC.restated("ftrl", seed)
    cond = SC.conditioning("ftrl", seed)
    print(c.describe("ftrl"))
    print("fp32 vs fp64: parameters %.3g  z %.3g (max |z| %.3g)  n %.3g (max n %.3g); near the threshold %s; zero-pattern mismatches %s; "
          "zero share v %.3f w %.3f" % (
              cond["param_gap"], cond["state_gaps"]["z"], max(np.abs(s64.z_w).max(), np.abs(s64.z_v).max() if s64.z_v.size else 0.0),
              cond["state_gaps"]["n"], max(s64.n_w.max(), s64.n_v.max() if s64.n_v.size else 0.0),
              " ".join("%s %d of %d" % (t, a, b) for t, (a, b) in cond["near"].items()), cond["zero_mismatch"],
              (m64.v == 0).mean() if m64.v.size else 0.0, (m64.w == 0).mean()))
    assert cond["ok"], "ill-conditioned case (replace the seed): " + "; ".join(cond["why"])
    assert SC.param_gap(m64, SC.start_model(c)) > 1e-4
