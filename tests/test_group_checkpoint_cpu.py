"""CPU: group checkpoints (fmx_group_checkpoint_save / _load) as far as they can be checked without a device: the
two declarations, their symbols and bindings, that the ABI version did not move, and the properties that make the shapes of
tests/test_gpu_group_checkpoint.py's kernel-edge tests edges, computed with the host form of the ownership rule (fmx_shard_place)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from group_checkpoint_cases import EDGE_CASES, MULTI_CHUNK, edge_ids, edge_properties, straddles

NEW = {
    "fmx_group_checkpoint_save": "int fmx_group_checkpoint_save(fmx_group g, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);",
    "fmx_group_checkpoint_load": "int fmx_group_checkpoint_load(fmx_group g, const char *path, const fmx_ckpt_opts *opts, fmx_ckpt_info *info /* may be NULL */);",
}


def header():
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        return f.read()


def test_the_two_functions_are_declared_bound_and_exported():
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
        assert hdr.index(decl) > hdr.index("} fmx_ckpt_info;")   # (C: the types it takes are declared before it)
    # the group forms take the per-handle forms' arguments behind the group: same options and info structs
    for call in ("save", "load"):
        assert bound["fmx_group_checkpoint_" + call] == bound["fmx_checkpoint_" + call], call
    # a NULL group is FMX_E_ARG without a device
    assert lib.fmx_group_checkpoint_save(None, b"x", None, None) == -1 and lib.fmx_group_checkpoint_load(None, b"x", None, None) == -1


def test_no_abi_or_format_version_change():
    from libfm_amd import build, capi, checkpoint
    build.build()
    assert int(re.search(r"#define\s+FMX_ABI_VERSION\s+(\d+)", header()).group(1)) == 11 == capi.load().fmx_abi_version()
    assert checkpoint.VERSION == 1


def test_group_binding_mirrors_the_handle():
    import inspect
    from libfm_amd import capi
    for name in ("checkpoint_save", "checkpoint_load"):
        assert callable(getattr(capi.Group, name))
        assert inspect.signature(getattr(capi.Group, name)) == inspect.signature(getattr(capi.Handle, name)), name


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_the_edge_cases_are_edges(name):
    from libfm_amd import build, capi
    build.build()
    n, k, world, shard_hash = EDGE_CASES[name]
    owner, local = capi.shard_place(n, world, shard_hash, np.arange(n, dtype=np.uint32))
    props = edge_properties(name, n, k, world, owner)
    print(name, owner.tolist(), props)
    assert len(props) >= 3 and all(props.values()), props
    ids = edge_ids(name, n, world, owner)
    assert 0 < len(ids) < n and (np.diff(ids.astype(np.int64)) > 0).all()
    # a member's local rows are dense: 0 .. count - 1, where count is what the library takes a member to own
    for r in range(world):
        mine = np.sort(local[owner == r])
        assert mine.tolist() == list(range((n - r + world - 1) // world if n > r else 0))


def test_between_them_the_edge_cases_cover_the_list():
    from libfm_amd import build, capi
    build.build()
    seen = set()
    for name, (n, k, world, shard_hash) in EDGE_CASES.items():
        owner, _ = capi.shard_place(n, world, shard_hash, np.arange(n, dtype=np.uint32))
        seen |= {p.split(":")[0] for p, ok in edge_properties(name, n, k, world, owner).items() if ok}
    for want in ("all members but one own a single row", "n is odd", "a w word holds features of two owners", "k is even", "k is 0",
                 "a state word straddles rows of two owners, dense", "the sparse list leaves out a member that owns rows"):
        assert want in seen, want


def test_the_multi_chunk_case_is_two_chunks_with_an_odd_tail():
    n, k, world, shard_hash = MULTI_CHUNK
    chunk = 16 << 20
    for cols in (k, k + 1):
        per = (chunk // (cols * 4)) & ~1                         # rows of a chunk: an even number (chunk_rows, csrc/fmx_ckpt.hip)
        assert per < n <= 2 * per and (n - per) % 2 == 1, cols
        assert chunk < n * cols * 4 < 2 * chunk
    assert n * 4 < chunk                                         # (w is one chunk)
    # (the helper on a case worked out by hand: rows of 3 elements, owners 0 1 0 1 -> elements 000 111 000 111, the word (0, 1))
    assert straddles(np.arange(4), 3, [0, 1, 0, 1]) and not straddles(np.arange(4), 2, [0, 1, 0, 1])
