"""FMX_SGD_SEQUENTIAL's dispatch, restated in plain Python (libfm_amd/csrc/fmx_sgd.hip: fmx_sgd_epoch, seq_runs_epoch, ensure_runs).

The mode is the reference's online loop (fm_learn_sgd_element.h:56-67) in every form it takes; which form, and which kernel instances,
depends on the slot's rows and on four switches the caller never sees.  cut_runs() is the greedy cut into conflict-free runs;
expected_route() names the status bits (include/fmx.h, ABI 9) and the kernel instances an epoch on that slot must run.  The tests
check the device against it (tests/test_gpu_sequential.py) and that their cases reach every form (tests/test_seq_routes.py)."""
import numpy as np

RUN_MAX = 4096          # ensure_runs: one wavefront evaluates a run's bias recurrence
RUN_ONE_MAX = 1024      # fmx_seq_kernels.h: a run of up to this many rows is ONE launch (k_run_fused)
RUN_FUSED_MAX = 2048    # ... up to this many TWO launches (k_rowsums + k_run_apply); longer ones three

STAT_SEQ_RUNS = 256
STAT_SEQ_ENTRIES, STAT_SEQ_WG, STAT_SEQ_ROWS, STAT_RUN_ONE, STAT_RUN_TWO, STAT_RUN_THREE = 1024, 2048, 4096, 8192, 16384, 32768
# the bits that say which form ran (a three-launch run also sets FMX_STAT_SCAN_PIT or _SCAN_SERIAL, by the device's occupancy: not checked)
SEQ_MASK = STAT_SEQ_RUNS | STAT_SEQ_ENTRIES | STAT_SEQ_WG | STAT_SEQ_ROWS | STAT_RUN_ONE | STAT_RUN_TWO | STAT_RUN_THREE

KNOBS = ("FMX_SEQ_RUNS", "FMX_SEQ_ROWS", "FMX_SEQ_WG", "FMX_SEQ_RUNS_FUSED", "FMX_SEQ_RUNS_ONE")


def kp_of(k):
    """the padded factor count the kernels are instantiated at: the next power of two (fmx_create)"""
    kp = 1
    while kp < max(int(k), 1):
        kp *= 2
    return kp


def row_flags(entries, row_ptr):
    """per row: (prev, rep).  prev = 1 + the latest earlier row that shares an id with it, 0: none; rep: the row repeats an id.
    The device sorts (id, row) keys and looks at neighbours (k_run_keys, k_run_prev); this is the same question."""
    rp = np.asarray(row_ptr, dtype=np.int64)
    n = len(rp) - 1
    prev = np.zeros(n, dtype=np.int64)
    rep = np.zeros(n, dtype=bool)
    ids = np.asarray(entries["id"], dtype=np.int64)
    if len(ids) == 0:
        return prev, rep
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    order = np.lexsort((row, ids))
    si, sr = ids[order], row[order]
    same = si[1:] == si[:-1]
    r, p = sr[1:][same], sr[:-1][same]
    rep[r[p == r]] = True
    np.maximum.at(prev, r[p != r], p[p != r] + 1)
    return prev, rep


def cut_runs(entries, row_ptr):
    """ensure_runs' greedy cut, in file order: a run ends in front of the first row that shares an id with a row of the run, in front of and
    behind a row that repeats an id (its own run, entry by entry), and at RUN_MAX rows.  Returns [(row0, n_rows, single)]."""
    prev, rep = row_flags(entries, row_ptr)
    n = len(prev)
    runs, start = [], 0
    for r in range(n):
        if rep[r]:
            if r > start:
                runs.append((start, r - start, False))
            runs.append((r, 1, True))
            start = r + 1
        elif (prev[r] > start and r > start) or r - start >= RUN_MAX:
            runs.append((start, r - start, False))
            start = r
    if start < n:
        runs.append((start, n - start, False))
    return runs


def _on(knobs, name):
    v = (knobs or {}).get(name)
    return not (v is not None and str(v)[:1] == "0")


def _zr(kp, max_row):
    """row slots of the k_run_fused instance (seq_runs_epoch): KP < 64 holds any row of <= 64 entries at ZR = KP; KP 64 / 128 take the
    smallest of 16 / 40 / 64 that holds the longest row; None: no instance (rows beyond the register path, or no such KP)"""
    if kp not in (8, 16, 32, 64, 128) or max_row > 64:
        return None
    if kp < 64:
        return kp
    return 16 if max_row <= 16 else 40 if max_row <= 40 else 64


def expected_route(k, k0, k1, task, max_row, runs, knobs=None):
    """what an FMX_SGD_SEQUENTIAL epoch on a slot must run.  runs: cut_runs() of the slot's rows; knobs: the environment of fmx_create
    (and of the epoch, for FMX_SEQ_RUNS).  k0 / k1 do not change the route (they are the kernels' runtime branches); they are taken so
    that a case list says everything an epoch depends on.  Returns (status bits & SEQ_MASK, set of kernel instances, number of runs or
    None when the epoch does not run as runs)."""
    del k0, k1
    kp = kp_of(k)
    n_rows = sum(nb for _, nb, _ in runs)
    sr = (knobs or {}).get("FMX_SEQ_RUNS")
    use_runs = n_rows > 0 and not (sr is not None and str(sr)[:1] == "0")
    if use_runs:
        use_runs = (sr is not None and str(sr)[:1] == "1") or n_rows >= 16 * len(runs)
    bits, inst = 0, set()
    has_rep = any(single for _, _, single in runs)
    if use_runs:
        bits |= STAT_SEQ_RUNS
        fused, one_env = _on(knobs, "FMX_SEQ_RUNS_FUSED"), _on(knobs, "FMX_SEQ_RUNS_ONE")
        zr = _zr(kp, max_row) if (fused and one_env) else None
        for _, nb, single in runs:
            if single:
                bits |= STAT_SEQ_ENTRIES
                inst.add("k_sequential<%d>" % kp)
            elif zr is not None and nb <= RUN_ONE_MAX:
                bits |= STAT_RUN_ONE
                inst.add("k_run_fused<%d,%d,%d>" % (kp, zr, task))
            elif fused and nb <= RUN_FUSED_MAX:
                bits |= STAT_RUN_TWO
                inst.add("k_rowsums<%d>" % kp)
                inst.add("k_run_apply<%d,%d>" % (kp, task))
            else:
                bits |= STAT_RUN_THREE
                inst.add("k_rowsums<%d>" % kp)
                inst.add("k_scan")
                inst.add("k_apply<%d>" % kp)
        return bits, inst, len(runs)
    rows_on, wg_on = _on(knobs, "FMX_SEQ_ROWS"), _on(knobs, "FMX_SEQ_WG")
    entries_fallback = max_row > 64 or has_rep             # (the row-at-a-time kernels run such rows entry by entry: seq_row_entries)
    if rows_on and wg_on and kp <= 128:
        bits |= STAT_SEQ_WG
        inst.add("k_sequential_wg<%d>" % (64 if kp <= 64 else 128))
    elif rows_on and kp <= 128:
        bits |= STAT_SEQ_ROWS
        inst.add("k_sequential_rows<%d,%d>" % (64 if kp <= 64 else 128, 64 if max_row > 32 else 32))
    else:
        bits |= STAT_SEQ_ENTRIES
        inst.add("k_sequential<%d>" % kp)
        entries_fallback = False
    if entries_fallback:
        inst.add("seq_row_entries<%d>" % kp)
    return bits, inst, None

