"""GPU: the route table of the SGD epoch drivers (libfm_amd/csrc/fmx_sgd.hip fmx_sgd_epoch / fmx_sgd_finish, fmx_comm.hip fmx_group_sgd_epoch).

One small configuration per route (tests/schedule_routes.py).  Each is held to
  * the epoch's counts -- batches, main_kernel_launches, deferred_features -- and the run-mode bits of its status (which form of the bias
    recurrence ran, one launch per batch or not, events or the device-side hand-off), as literals: what the drivers reported before their
    per-mode bodies were split into functions (profiles/epoch_fingerprint_before.jsonl; scripts/epoch_fingerprint.py compares the parameters
    bit for bit, this file does not);
  * no fall-back: FMX_STAT_SCAN_FALLBACK and FMX_STAT_HANDOFF_TIMEOUT absent;
  * the oracle's rule after the configuration's epochs, at the tolerance tests/test_gpu_parity.py (test_gpu_group.py, test_gpu_sgda.py) holds
    the same rule to -- so that a route cannot keep its counts and compute something else.
FMX_STAT_EVENT_SYNC is not looked at where the bias lag is >= 2 at batches >= 32 768: there it says whether the device ran the handle's two
streams side by side when the epoch asked.  FMX_APPLY_STORE with ids that collide inside a batch, HOGWILD and FMX_APPLY_ATOMIC have no oracle
(include/fmx.h: their numbers depend on the order of the wavefronts; when the table was recorded FMX_APPLY_STORE did not reproduce its own
parameters from one run to the next): counts, status and finite parameters only."""
import numpy as np
import pytest

import schedule_routes as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4
PIT, SERIAL, EVENTS, ONE = R.STAT_SCAN_PIT, R.STAT_SCAN_SERIAL, R.STAT_EVENT_SYNC, R.STAT_SMALL_ONE

# config -> (batches, main_kernel_launches, deferred_features, run-mode bits)
EXPECTED = {
    "fused_side_handoff_lag2":   (3, 3, 39573, PIT | SERIAL),            # (the short last batch takes the chain)
    "fused_side_events_lag1":    (3, 3, 39573, PIT | SERIAL | EVENTS),
    "fused_two_launches_b2048":  (3, 3, 2844, SERIAL),
    "fused_small_one_b512":      (3, 3, 215, SERIAL | ONE),
    "fused_small_one_off_b512":  (3, 3, 215, SERIAL),
    "fused_keep_wside_b512":     (3, 3, 215, SERIAL | ONE),
    "fused_chunk48_serial_scan": (3, 3, 39573, SERIAL),
    "fused_chunk256_tiled_scan": (3, 3, 39573, SERIAL),
    "fused_small_one_k64":       (3, 3, 215, SERIAL | ONE),
    "default_b2048":             (3, 0, 0, SERIAL),
    "default_lag_b2048":         (3, 0, 0, SERIAL),
    "segmented_b2048":           (3, 0, 0, SERIAL),
    "segmented_lag_b2048":       (3, 0, 0, SERIAL),
    "store_b2048":               (3, 0, 0, SERIAL),
    "store_lag_b2048":           (3, 0, 0, SERIAL),
    "segmented_masked_nnz24":    (3, 0, 0, SERIAL),
    "default_lag_k64":           (3, 0, 0, SERIAL),
    "sgda_minibatch":            (3, 3, 0, 0),
    "group_in_stream_b512":      (3, 3, 0, SERIAL),
    "group_general_b512":        (3, 3, 0, SERIAL),
    "group_pipeline_b512":       (3, 3, 0, SERIAL),
    "group_side_b40000_lag2":    (3, 3, 0, PIT | SERIAL),
    "group_exact_b512":          (3, 3, 0, SERIAL),
    "hogwild_store":             (3, 3, 0, SERIAL),
    "minibatch_atomic_b2048":    (3, 0, 0, SERIAL),
}


@pytest.fixture(scope="module")
def capi():
    from libfm_amd import build, capi
    build.build()
    if capi.load().fmx_device_count() == 0:
        pytest.fail("gpu-marked test without a HIP device")
    return capi


_ORACLE = {}


def oracle_model(O, c, chunk_used):
    """the oracle's parameters for `c`, computed once per rule (several routes run the same rule) and left unchanged"""
    lag = (c["lag"] or 1) if (c["apply"] == R.FUSED or c["flags"] & R.FLAG_BIAS_LAG) else 0
    key = (c["kind"] == "sgda", c["k"], c["rows"], c["nnz"], c["batch"], chunk_used, lag, bool(c["flags"] & R.FLAG_PIPELINE), c["epochs"])
    if key not in _ORACLE:
        _ORACLE[key] = R.oracle_params(O, c, chunk_used)
    return _ORACLE[key]


def test_every_configuration_has_its_row():
    assert sorted(EXPECTED) == sorted(R.BY_NAME)


@pytest.mark.parametrize("name", [c["name"] for c in R.CONFIGS])
def test_route(capi, oracle, name):
    c = R.BY_NAME[name]
    st, (w0, w, v) = R.run(capi, c)
    batches, launches, deferred, bits = EXPECTED[name]
    print(name, int(st.batches), int(st.main_kernel_launches), int(st.deferred_features), hex(int(st.status)))
    assert st.batches == batches == (c["rows"] + c["batch"] - 1) // c["batch"]
    assert st.main_kernel_launches == launches
    assert st.deferred_features == deferred
    assert R.route_bits(c, st.status) == bits & ~(EVENTS if R.event_sync_masked(c) else 0), hex(int(st.status))
    assert not st.status & (R.STAT_SCAN_FALLBACK | R.STAT_HANDOFF_TIMEOUT), hex(int(st.status))
    if not c["oracle"]:
        assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all()
        return
    chunk = c["chunk"] if c["kind"] == "sgda" else int(st.w0_chunk_used)
    assert chunk == (c["chunk"] or capi.default_w0_chunk(R.LR, capi.TASK_CLASSIFICATION))
    m = oracle_model(oracle, c, chunk)
    atol = 2e-5 if c["kind"] == "sgda" else 1e-5          # (tests/test_gpu_sgda.py; tests/test_gpu_parity.py and test_gpu_group.py)
    assert abs(w0 - m.w0) <= RTOL * abs(m.w0) + atol
    np.testing.assert_allclose(w, m.w, rtol=RTOL, atol=atol)
    np.testing.assert_allclose(v, m.v, rtol=RTOL, atol=atol)
