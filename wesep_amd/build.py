"""Build libwesep_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m wesep_amd.build [--force]
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libwesep_hip.so")
OBJ = os.path.join(CSRC, "_obj")
# No packed FP32 instructions (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32) in this library: on the MI355X a packed FP32
# op whose src1 selects the other half (op_sel -- what hipcc emits for complex arithmetic and 2-vector swizzles) returns
# wrong low halves while gemm_b2p / the grouped gemm_nt / gemm_tn run on the same CU from another stream
# (profiles/r03_kernel_race.md; standalone reproducer tools/cbench/race_repro.hip).  The scalar forms are not affected.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + NO_PACKED_FP32


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "hipcc")
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + \
        [os.path.join(os.path.dirname(HERE), "include", "wesep_hip.h")]
    os.makedirs(OBJ, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
        if force or _stale(obj, [src] + hdrs):
            cmd = [hipcc] + FLAGS + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            # the feature flag reaches the host pass too, which says it does not know it: not worth showing 17 times
            err = "\n".join(ln for ln in r.stderr.splitlines() if "'-packed-fp32-ops' is not a recognized feature" not in ln)
            if err.strip():
                print(err, file=sys.stderr, flush=True)
            if r.returncode:
                raise subprocess.CalledProcessError(r.returncode, cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(compile_one, srcs))
    if force or _stale(OUT, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", OUT]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


RUNTIME = os.path.join(os.path.dirname(HERE), "runtime")
ENGINE_OUT = os.path.join(RUNTIME, "libwesep_engine.so")
MAIN_OUT = os.path.join(RUNTIME, "separate_main")
# libwesep_engine.so: one translation unit per part (runtime/engine_internal.h); it exports the C ABI only
ENGINE_SRCS = ["engine.cc", "speaker.cc", "bsrnn_plan.cc", "tasnet_plan.cc", "dpccn_plan.cc", "gridnet_plan.cc",
               "longform.cc", "live.cc", "live_pool.cc", "tail_pool.cc", "rate_tail_pool.cc", "stream.cc", "stream_pool.cc", "rate.cc", "rate_pool.cc"]


def build_runtime(force=False, verbose=True):
    """libwesep_engine.so (native inference runtime over the C ABI, include/wesep_engine.h) and the `separate_main`
    command-line tool.  Host code only; links libwesep_hip.so (built first)."""
    hipcc = os.environ.get("HIPCC", "hipcc")
    inc = os.path.join(os.path.dirname(HERE), "include")
    deps = [os.path.join(RUNTIME, f) for f in ENGINE_SRCS + ["engine_internal.h", "wav_io.h", "separate_main.cc"]] + \
        [os.path.join(inc, "wesep_engine.h"), os.path.join(inc, "wesep_hip.h"), OUT]
    cmds = []
    if force or _stale(ENGINE_OUT, deps):
        cmds.append([hipcc, "-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-shared"] +
                    [os.path.join(RUNTIME, f) for f in ENGINE_SRCS] +
                    ["-o", ENGINE_OUT, "-L" + HERE, "-lwesep_hip", "-Wl,-rpath,$ORIGIN/../wesep_amd"])
    if force or _stale(MAIN_OUT, deps + [ENGINE_OUT]) or cmds:
        cmds.append([hipcc, "-O2", "-std=c++17", "-pthread", os.path.join(RUNTIME, "separate_main.cc"), "-o", MAIN_OUT,
                     "-L" + RUNTIME, "-lwesep_engine", "-L" + HERE, "-lwesep_hip", "-Wl,-rpath,$ORIGIN",
                     "-Wl,-rpath,$ORIGIN/../wesep_amd"])
    bench_src = os.path.join(os.path.dirname(HERE), "tools", "cbench", "lstm_bench.cc")
    bench_out = bench_src[:-3]
    if os.path.exists(bench_src) and (force or _stale(bench_out, [bench_src, OUT, os.path.join(inc, "wesep_hip.h")])):
        cmds.append([hipcc, "-O2", "-std=c++17", bench_src, "-o", bench_out, "-L" + HERE, "-lwesep_hip",
                     "-Wl,-rpath,$ORIGIN/../../wesep_amd"])      # Python-free microbenchmark (tools/cbench)
    race_src = os.path.join(os.path.dirname(HERE), "tools", "cbench", "race_repro.hip")
    race_out = race_src[:-4]
    clone_src = os.path.join(os.path.dirname(race_src), "b2p_clone.hip")
    if os.path.exists(race_src) and (force or _stale(race_out, [race_src, clone_src, OUT, os.path.join(inc, "wesep_hip.h")])):
        # standalone reproducer of the packed-FP32 disturbance (profiles/r03_kernel_race.md); its victims are meant to
        # contain packed FP32 instructions, so it is NOT compiled with the library's NO_PACKED_FP32 -- the restated
        # aggressor (b2p_clone.hip: gemm_b2p with one ingredient removable at a time) is, like the library itself
        clone_obj = os.path.join(os.path.dirname(race_src), "b2p_clone.o")
        cmds.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *NO_PACKED_FP32, "-c", clone_src, "-o", clone_obj])
        race_obj = race_out + ".o"
        cmds.append([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-c", race_src, "-o", race_obj])
        cmds.append([hipcc, "--offload-arch=gfx950", race_obj, clone_obj, "-o", race_out, "-L" + HERE,
                     "-lwesep_hip", "-Wl,-rpath,$ORIGIN/../../wesep_amd"])
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return ENGINE_OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_runtime(force="--force" in sys.argv)
    print("built", OUT, ENGINE_OUT, MAIN_OUT)
