"""Build recipe of the HIP library: libfm_amd/libfmx.so (gfx950 only, in-tree so it travels with gpurun).

    python -m libfm_amd.build [--force]

Twenty-two translation units (csrc/fmx_core.hip, fmx_sgd.hip, fmx_als.hip, fmx_io.hip, fmx_comm.hip, fmx_pair.hip, fmx_topk.hip,
fmx_pairneg.hip, fmx_eval.hip, fmx_post.hip, fmx_evalq.hip, fmx_compact.hip, fmx_rankq.hip, fmx_mem.hip, fmx_weighted.hip, fmx_ckpt.hip, fmx_snap.hip, fmx_fwfm.hip, fmx_ffm.hip, fmx_fmfm.hip, fmx_hofm.hip, fmx_dfm.hip) are compiled in parallel and linked.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SRC = [os.path.join(CSRC, f) for f in ("fmx_core.hip", "fmx_sgd.hip", "fmx_als.hip", "fmx_io.hip", "fmx_comm.hip", "fmx_pair.hip", "fmx_topk.hip", "fmx_pairneg.hip", "fmx_eval.hip", "fmx_post.hip", "fmx_evalq.hip", "fmx_compact.hip", "fmx_rankq.hip", "fmx_mem.hip", "fmx_weighted.hip", "fmx_ckpt.hip", "fmx_snap.hip", "fmx_fwfm.hip", "fmx_ffm.hip", "fmx_fmfm.hip", "fmx_hofm.hip", "fmx_dfm.hip")]
DEPS = SRC + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(ROOT, "include", "fmx.h")]   # every header under csrc/
# experiments: FMX_DEFS="-DFMX_V_NT=1" FMX_OUT=libfmx_nt.so python -m libfm_amd.build --force ; run with FMX_LIB=<that file>
EXTRA = os.environ.get("FMX_DEFS", "").split()
OUT = os.path.join(HERE, os.environ.get("FMX_OUT", "libfmx.so"))
OBJ_DIR = os.path.join(HERE, "build" + ("_" + os.environ["FMX_OUT"].replace(".", "_") if "FMX_OUT" in os.environ else ""))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fPIC", "-fvisibility=hidden",
         "-Wno-unused-result", "-Wno-unused-value"]
# per file.  fmx_fwfm.hip is compiled without the packed fp32 instructions (v_pk_add / mul / fma_f32): every fp32 operation of its
# kernels is then one scalar instruction, and the unit needs fewer registers for it -- k_fwfm_rows<64, 4, true> 152 VGPRs against 212,
# <128, 4, true> 156 against 260, scratch 0 either way.  It is an internal clang feature switch (the host pass
# prints "not a recognized feature" for it): should a compiler drop it, removing the entry costs occupancy, not correctness.  The
# unit's instance of stateful_seg_block (k_fwfm_apply_seg) is compiled this way too; fmx_sgd.hip's instances are not touched.
# fmx_ffm.hip is compiled the same way (its resource table is in DESIGN.md section 30).
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FILE_FLAGS = {"fmx_fwfm.hip": NO_PACKED_FP32, "fmx_ffm.hip": NO_PACKED_FP32}


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = [os.path.join(OBJ_DIR, os.path.basename(s)[:-4] + ".o") for s in SRC]

    def cc(pair):
        cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(os.path.basename(pair[0]), []) + EXTRA + ["-c", pair[0], "-o", pair[1]]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(len(SRC)) as ex:
        list(ex.map(cc, zip(SRC, objs)))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", OUT]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
