"""Build the HIP extension (librs_hip.so) in-tree for gfx950 with hipcc.  No torch headers are
involved: the library is a plain C-ABI shared object (include/radsearch.h).  Each translation unit is
compiled to an object (in parallel, rebuilt only when one of its inputs changed) and linked."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "librs_hip.so")

SOURCES = ["rs_env.hip", "rs_ppo.hip", "rs_maps.hip", "rs_cnn.hip", "rs_cnn_sized.hip", "rs_pfgru.hip", "rs_gru.hip", "rs_pfgru_train.hip", "rs_rnn_policy.hip", "rs_welford.hip", "rs_cnn_loss.hip",
           "rs_rnn_sized.hip", "rs_pfgru_sized.hip", "rs_pfgru_sized_train.hip", "rs_ff_team.hip", "rs_eval.hip", "rs_draws.hip", "rs_cnn_eval.hip", "rs_lookahead.hip", "rs_bpf.hip"]
# -ffp-contract=off: float64 env arithmetic must round like the reference's Python floats (no FMA fusing)
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
          "-Wno-unused-function"]
# rs_ppo.hip: no SLP packing.  hipcc otherwise pairs the scalar f32 FMAs of the output layer into v_pk_fma_f32 + v_mov shuffles,
# which costs more issue slots than it saves next to f32 MFMAs (measured: scripts/micro/mfma_valu_coissue.hip)
# rs_ff_team.hip, rs_eval.hip: the same output layer (rs_mlp.hpp) next to the same MFMAs, the same flag
# rs_rnn_sized.hip: the 64-unit tier's unrolled block loops exceed the default full-unroll budget; left rolled, the register arrays they
# index go to scratch (528 bytes per lane at 64 units)
EXTRA_CFLAGS = {"rs_ppo.hip": ["-fno-slp-vectorize"], "rs_ff_team.hip": ["-fno-slp-vectorize"], "rs_eval.hip": ["-fno-slp-vectorize"],
                "rs_rnn_sized.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"],
                "rs_pfgru_sized.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"]}


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the MI355X extension cannot be built")


def _deps():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "include", "radsearch.h"), __file__]


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True, defines=(), suffix: str = "") -> str:
    """defines / suffix: a diagnostic variant next to the product library, e.g. build(defines=["RS_K7_STAMPS"],
    suffix="_stamps") -> lib/librs_hip_stamps.so (selected with RS_LIB_PATH; see scripts/k7_stamps.py).
    --skew [--prio N] on the command line: -DRS_K7_SKEW (the partner-gap table of scripts/k7_partner_gap.py, no phase stamps)
    with the priority rule RS_K7_PRIO=N of rs_ppo_grad2.hpp -> lib/librs_hip_skew[_prioN].so; --prio N alone: the product
    kernels with that rule -> lib/librs_hip_prioN.so."""
    deps = _deps()
    lib = LIB.replace(".so", suffix + ".so")
    if not force and not _newer(lib, deps):
        return lib
    os.makedirs(OBJDIR, exist_ok=True)
    cc = hipcc()

    def compile_one(src):
        obj = os.path.join(OBJDIR, src.replace(".hip", suffix + ".o"))
        if force or _newer(obj, deps):
            cmd = [cc] + CFLAGS + EXTRA_CFLAGS.get(src, []) + ["-D" + d for d in defines] + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print("[radiation_ppo_amd.build]", " ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        return obj

    # as many compilers at once as there are CPUs to run them (MAX_JOBS caps it where set), the two slowest translation units first
    # (~70 and ~45 s; the others 2-15 s): one compiler per source at once needs ~2.5 GB on a small build machine for no gain in time
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    jobs = max(1, min(len(SOURCES), cpus, int(os.environ.get("MAX_JOBS") or cpus)))
    order = sorted(SOURCES, key=lambda f: f not in ("rs_rnn_sized.hip", "rs_pfgru_sized.hip"))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        done = dict(zip(order, ex.map(compile_one, order)))
    objs = [done[f] for f in SOURCES]
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib]
    if verbose:
        print("[radiation_ppo_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return lib


if __name__ == "__main__":
    prio = sys.argv[sys.argv.index("--prio") + 1] if "--prio" in sys.argv else None
    if "--stamps" in sys.argv:
        build(force="--force" in sys.argv, defines=["RS_K7_STAMPS"], suffix="_stamps")
    elif "--skew" in sys.argv or prio is not None:
        skew = "--skew" in sys.argv
        build(force="--force" in sys.argv, defines=(["RS_K7_SKEW"] if skew else []) + ([f"RS_K7_PRIO={int(prio)}"] if prio is not None else []),
              suffix=("_skew" if skew else "") + (f"_prio{int(prio)}" if prio is not None else ""))
    else:
        build(force="--force" in sys.argv)
