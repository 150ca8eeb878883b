"""The shapes of the kernel-edge tests of the group checkpoint (tests/test_gpu_group_checkpoint.py) and the property that makes each
one an edge, as host arithmetic over the ownership rule (capi.shard_place): tests/test_group_checkpoint_cpu.py asserts the
properties without a device, the GPU test asserts them again before it uses a case.

A section is streamed as 8-byte words of two 4-byte elements; a row of a section has `cols` elements (w: 1, V: k, a state table: k + 1).
The group's kernels filter per ELEMENT because the two elements of a word can belong to rows of different owners."""
import numpy as np

# name -> (n, k, world, shard_hash)
EDGE_CASES = {
    "n9_w8": (9, 2, 8, 1),           # seven members own ONE row (fmx_create refuses more shards than features, so none owns nothing);
                                     # n odd; k even: a state row has 3 elements
    "n9_w8_k0": (9, 0, 8, 1),        # k = 0: no V section, a state row is the linear coordinate alone
    "n37_w3": (37, 2, 3, 1),         # every member owns rows; hashed
    "n38_w2_plain": (38, 3, 2, 0),   # unhashed: neighbours alternate between the two members; k odd
}
MULTI_CHUNK = (70001, 64, 3, 1)      # V and each FTRL table are two 16 MiB chunks, the second with an odd row count


def edge_ids(name, n, world, owner):
    """the id list of the case's sparse file: every feature but those of the member that owns feature 0 -- a member that owns rows
    and contributes none"""
    return np.array([j for j in range(n) if owner[j] != owner[0]], dtype=np.uint32)


def straddles(rows, cols, owner):
    """does a word of a section whose rows are the features `rows`, `cols` elements each, hold elements of two owners?"""
    elem_owner = np.repeat(np.asarray(owner)[np.asarray(rows, dtype=np.int64)], cols)
    pairs = elem_owner[:len(elem_owner) // 2 * 2].reshape(-1, 2)
    return bool((pairs[:, 0] != pairs[:, 1]).any())


def edge_properties(name, n, k, world, owner):
    """{property: holds} of a case; every value must be True"""
    owner = np.asarray(owner)
    counts = np.bincount(owner, minlength=world)
    ids = edge_ids(name, n, world, owner)
    every = np.arange(n)
    props = {
        "a w word holds features of two owners": straddles(every, 1, owner),
        "the sparse list leaves out a member that owns rows": len(ids) > 0 and counts[owner[0]] > 0 and not (owner[ids] == owner[0]).any(),
    }
    if k > 0 and k % 2 == 0:                                     # (an odd number of elements per state row: words straddle rows)
        props["a state word straddles rows of two owners, dense"] = straddles(every, k + 1, owner)
        props["a state word straddles rows of two owners, sparse"] = straddles(ids, k + 1, owner)
    if name.startswith("n9_w8"):
        props["all members but one own a single row"] = sorted(counts.tolist()) == [1] * (world - 1) + [2]
        props["n is odd: the last word of w is half padding"] = n % 2 == 1
    if name == "n9_w8":
        props["k is even: a state row has an odd number of elements"] = k % 2 == 0 and k > 0
    if name == "n9_w8_k0":
        props["k is 0"] = k == 0
    if name == "n37_w3":
        props["every member owns rows"] = bool((counts > 0).all())
    if name == "n38_w2_plain":
        props["unhashed: owner is id mod world"] = bool((owner == every % world).all())
    return props
