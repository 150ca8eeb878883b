"""CPU: AdaGrad and FTRL over feature shards (fmx_group_adapt_* / fmx_group_ftrl_* / fmx_group_param_sparsity) as
far as it goes without a device: the nine functions stand in include/fmx.h, in capi's table and in libfmx.so's dynamic symbols under
their C names; the ABI version stays 11; the learner and the command line refuse what has no sharded form before any device is
touched.  The device side is tests/test_gpu_group_stateful.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = {
    "fmx_group_adapt_begin": "int fmx_group_adapt_begin(fmx_group g, const fmx_adapt_opts *opts);",
    "fmx_group_adapt_epoch": "int fmx_group_adapt_epoch(fmx_group g, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);",
    "fmx_group_adapt_get_state_rows": "int fmx_group_adapt_get_state_rows(fmx_group g, const uint32_t *ids, uint32_t count, double *nw_out, double *nv_out);",
    "fmx_group_adapt_end": "int fmx_group_adapt_end(fmx_group g);",
    "fmx_group_ftrl_begin": "int fmx_group_ftrl_begin(fmx_group g, const fmx_ftrl_opts *opts);",
    "fmx_group_ftrl_epoch": "int fmx_group_ftrl_epoch(fmx_group g, int slot, uint32_t batch, uint32_t w0_chunk, fmx_epoch_stats *stats);",
    "fmx_group_ftrl_get_state_rows": "int fmx_group_ftrl_get_state_rows(fmx_group g, const uint32_t *ids, uint32_t count, double *zw, double *zv, double *nw, double *nv);",
    "fmx_group_ftrl_end": "int fmx_group_ftrl_end(fmx_group g);",
    "fmx_group_param_sparsity": "int fmx_group_param_sparsity(fmx_group g, fmx_sparsity *out);",
}


def header():
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        return f.read()


def test_the_nine_functions_are_declared_bound_and_exported():
    from libfm_amd import build, capi
    build.build()
    hdr = header()
    bound = {name: (res, args) for name, res, args in capi.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libfm_amd", "libfmx.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = capi.load()
    for name, decl in NEW.items():
        assert decl in hdr, name
        assert [n for n, _, _ in capi.SYMBOLS].count(name) == 1, name
        assert name in exported, name                           # unmangled => extern "C"
        assert hasattr(lib, name), name
    # the group forms take the per-handle forms' arguments behind the group: same options and stats structs, same output arrays
    for rule in ("adapt", "ftrl"):
        for call in ("begin", "epoch", "get_state_rows", "end"):
            assert bound["fmx_group_%s_%s" % (rule, call)] == bound["fmx_%s_%s" % (rule, call)], (rule, call)
    assert bound["fmx_group_param_sparsity"] == bound["fmx_param_sparsity"]


def test_abi_version_stays_11():
    from libfm_amd import build, capi
    build.build()
    assert int(re.search(r"#define\s+FMX_ABI_VERSION\s+(\d+)", header()).group(1)) == 11 == capi.load().fmx_abi_version()


def test_group_binding_mirrors_the_handle():
    from libfm_amd import capi
    for name in ("adapt_begin", "adapt_epoch", "adapt_state_rows", "adapt_end", "ftrl_begin", "ftrl_epoch", "ftrl_state_rows", "ftrl_end",
                 "param_sparsity"):
        assert callable(getattr(capi.Group, name)) and callable(getattr(capi.Handle, name)), name


def sharded_learner(optimizer="adagrad", devices=(0, 0)):
    from libfm_amd import learner as L
    l = L.FMLearnSGD()
    l.fm = L.FMModel()
    l.fm.num_attribute, l.fm.num_factor = 10, 2
    l.fm.init()
    l.learn_rate, l.task, l.optimizer, l.devices = 0.01, L.TASK_CLASSIFICATION, optimizer, list(devices)
    return l


def some_data():
    from libfm_amd import capi, learner as L
    ent = np.zeros(4, dtype=capi.ENTRY_DTYPE)
    ent["id"], ent["value"] = [0, 1, 2, 3], 1.0
    return L.Data(ent, np.array([0, 2, 4], dtype=np.uint64), np.array([1.0, -1.0], dtype=np.float32))


def test_learner_refuses_plain_sgd_on_shards_before_any_device():
    l = sharded_learner("sgd")
    with pytest.raises(NotImplementedError, match="optimizer sgd is not supported on feature shards"):
        l.init()
    assert l._h is None and l._shards == []
    with pytest.raises(NotImplementedError, match="feature shards"):
        l.learn(some_data(), some_data())


@pytest.mark.parametrize("optimizer", ["adagrad", "ftrl"])
def test_learner_refuses_what_has_no_sharded_form_before_any_device(optimizer, tmp_path):
    """compact, recommend, the checkpoints and row weights on a sharded learner: NotImplementedError from the `devices` field alone --
    none of them gets as far as a handle (there is none: init() has not run)"""
    l = sharded_learner(optimizer)
    d = some_data()
    for call in (lambda: l.compact(), lambda: l.compact("int8", prune="dead"), lambda: l.recommend(d, d, 1),
                 lambda: l.save_checkpoint(str(tmp_path / "a.ckpt")), lambda: l.load_checkpoint(str(tmp_path / "no_such.ckpt")),
                 lambda: l.set_weights(d, np.ones(2))):
        with pytest.raises(NotImplementedError, match="not supported on feature shards"):
            call()
    assert l._h is None
    l.set_weights(d, None)                                      # (dropping weights that were never there stays harmless)


def test_one_device_in_the_list_is_one_handle():
    """devices with one entry is not sharded: nothing is refused on its account"""
    l = sharded_learner("sgd", devices=(0,))
    assert not l._sharded()
    with pytest.raises(ValueError, match="before init"):
        l.save_checkpoint("x")
    l = sharded_learner("sgd", devices=())
    assert not l._sharded()
    from libfm_amd import learner as L
    assert L.FMLearnSGD().devices is None


def test_pairwise_and_sgda_learners_have_no_sharded_form():
    from libfm_amd import learner as L
    for cls in (L.FMLearnPairSGD, L.FMLearnPairAdaptive, L.FMLearnSGDA):
        l = cls()
        l.fm = L.FMModel()
        l.fm.num_attribute, l.fm.num_factor = 10, 2
        l.fm.init()
        l.learn_rate, l.devices = 0.01, [0, 0]
        if cls is L.FMLearnPairAdaptive:
            l.optimizer = "adagrad"
        with pytest.raises(NotImplementedError, match="feature shards"):
            l.init()
        assert l._h is None


BASE = ["-task", "c", "-train", "no_such_train", "-test", "no_such_test", "-learn_rate", "0.01"]


@pytest.mark.parametrize("argv, text", [
    (["-method", "sgd", "-devices", "0,0"], "ERROR: -devices belongs to -method sgd with -optimizer adagrad or ftrl: -method sgd -optimizer sgd has no form on feature shards"),
    (["-method", "als", "-devices", "0,0"], "-method als has no form on feature shards"),
    (["-method", "mcmc", "-devices", "0,0"], "-method mcmc has no form on feature shards"),
    (["-method", "sgda", "-devices", "0,0"], "-method sgda has no form on feature shards"),
    (["-method", "bpr", "-train_pairs", "p", "-test_pairs", "q", "-optimizer", "adagrad", "-devices", "0,0"], "-method bpr -optimizer adagrad has no form on feature shards"),
    (["-method", "sgd", "-optimizer", "adagrad", "-devices", "0,0", "-serve", "bf16"], "ERROR: -serve is not supported with -devices"),
    (["-method", "sgd", "-optimizer", "ftrl", "-devices", "0,0", "-topk", "3", "-candidates", "c"], "ERROR: -topk is not supported with -devices"),
    (["-method", "sgd", "-optimizer", "ftrl", "-devices", "0,0", "-save_checkpoint", "x"], "ERROR: -save_checkpoint is not supported with -devices"),
    (["-method", "sgd", "-optimizer", "adagrad", "-devices", "0,0", "-load_checkpoint", "x"], "ERROR: -load_checkpoint is not supported with -devices"),
    (["-method", "sgd", "-optimizer", "adagrad", "-devices", "0,0", "-train_weights", "x"], "ERROR: -train_weights is not supported with -devices"),
    (["-method", "sgd", "-optimizer", "adagrad", "-devices", "a,b"], "ERROR: -devices needs 1 .. 16 device ordinals"),
    (["-method", "sgd", "-optimizer", "adagrad", "-devices", ""], "ERROR: -devices needs 1 .. 16 device ordinals"),
])
def test_cli_refuses_before_any_device(argv, text, capsys):
    from libfm_amd import cli
    assert cli.main(BASE + argv) == 0
    assert text in capsys.readouterr().err


def test_cli_help_lists_the_flag(capsys):
    from libfm_amd import cli
    cli.main(["-help"])
    assert "-devices" in capsys.readouterr().out
