"""Builds the HIP engine in-tree: bayesian_dlms_amd/libdlm_engine.so (gfx950 only)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdlm_engine.so")
SOURCES = ["dlm_engine.hip", "dlm_generic.hip", "dlm_mfma16.hip", "dlm_sparse16.hip", "dlm_sampler16.hip", "dlm_tiled.hip", "dlm_wave48.hip", "dlm_svd.hip", "dlm_ar1.hip", "dlm_lane.hip", "dlm_gibbs.hip", "dlm_loglik.hip", "dlm_studentt.hip", "dlm_sv.hip", "dlm_sv_ou.hip", "dlm_sv_knots.hip", "dlm_fsv.hip", "dlm_dlmfsv.hip", "dlm_fsv_forecast.hip", "dlm_pf.hip", "dlm_storvik.hip", "dlm_lw.hip", "dlm_rb.hip", "dlm_pg.hip", "dlm_pf_forecast.hip", "dlm_pf_forecast_learned.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
FLAGS = BASE_FLAGS + ["-mllvm", "-amdgpu-mfma-vgpr-form"]
# dlm_wave48.hip keeps whole matrices in registers (up to the 512-register budget of a wave): its accumulators may live
# in AGPRs, and the VGPR-form rewrite pass of this compiler crashes on it
FILE_FLAGS = {"dlm_wave48.hip": BASE_FLAGS}
# an object is stale when its source or any of these is newer (dlm_wave.h: the device primitives of the kernel files; dlm_draws.h: the draws of the Gibbs parameter steps; dlm_pf_common.h: what the particle kernels share; dlm_obs_draws.h: the forecast kernels' observation draws and sort)
HEADERS = [os.path.join(CSRC, "dlm_internal.h"), os.path.join(CSRC, "dlm_wave.h"), os.path.join(CSRC, "dlm_draws.h"), os.path.join(CSRC, "dlm_pf_common.h"), os.path.join(CSRC, "dlm_obs_draws.h"), os.path.join(CSRC, "dlm_fsv_solve.h"), os.path.join(HERE, "..", "include", "dlm_engine.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_all(todo, verbose):
    """Runs the compile commands side by side: the translation units are independent (the largest takes about two minutes)."""
    if not todo:
        return
    from concurrent.futures import ThreadPoolExecutor
    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(len(todo), max(1, (os.cpu_count() or 2) // 2))) as pool:
        list(pool.map(run, todo))


def build_variant(name, defines):
    """Experimental build with extra -D flags -> bayesian_dlms_amd/libdlm_engine_<name>.so."""
    out = os.path.join(HERE, f"libdlm_engine_{name}.so")
    objs = []
    os.makedirs(os.path.join(HERE, "build", name), exist_ok=True)
    for src in SOURCES:
        o = os.path.join(HERE, "build", name, src.replace(".hip", ".o"))
        subprocess.check_call([HIPCC] + FILE_FLAGS.get(src, FLAGS) + [f"-D{d}" for d in defines] + ["-c", os.path.join(CSRC, src), "-o", o])
        objs.append(o)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-L/opt/rocm/lib", "-lrccl"])
    return out


def build_tu_variant(name, srcs, defines):
    """Experimental build in which only the named translation unit(s) get extra -D flags (the other objects come from the regular
    build) -> bayesian_dlms_amd/libdlm_engine_<name>.so.  `srcs`: one source file name or a list of them.  Select it with DLM_ENGINE_LIB."""
    build()
    srcs = [srcs] if isinstance(srcs, str) else list(srcs)
    out = os.path.join(HERE, f"libdlm_engine_{name}.so")
    own = {src: os.path.join(HERE, "build", f"{name}_{src.replace('.hip', '.o')}") for src in srcs}
    for src, o in own.items():
        subprocess.check_call([HIPCC] + FILE_FLAGS.get(src, FLAGS) + [f"-D{d}" for d in defines] + ["-c", os.path.join(CSRC, src), "-o", o])
    objs = [own.get(s, os.path.join(HERE, "build", s.replace(".hip", ".o"))) for s in SOURCES]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-L/opt/rocm/lib", "-lrccl"])
    return out


# The translation units whose LDS-DMA prefetches are waited for by hand count (vm_wait in csrc/dlm_internal.h)
DRAIN_SOURCES = ["dlm_sparse16.hip", "dlm_sampler16.hip", "dlm_svd.hip"]
DRAIN_LIB = os.path.join(HERE, "libdlm_engine_drain.so")


def drain_object(src):
    return os.path.join(HERE, "build", "drain", src.replace(".hip", ".o"))


def build_drain_variant(force=False, verbose=False):
    """The engine with every hand-counted wait drained (-DDLM_DRAIN_WAITS=1: vmcnt(0)) -> bayesian_dlms_amd/libdlm_engine_drain.so.
    Only the DRAIN_SOURCES are compiled again; the other objects are the regular build's.  Rebuilt only when a source or header
    is newer, as build() does.  tests/test_counted_waits_gpu.py compares it with the default build bit for bit."""
    build(verbose=verbose)
    os.makedirs(os.path.join(HERE, "build", "drain"), exist_ok=True)
    todo = []
    for src in DRAIN_SOURCES:
        s, o = os.path.join(CSRC, src), drain_object(src)
        if force or _stale(o, [s] + HEADERS):
            todo.append([HIPCC] + FILE_FLAGS.get(src, FLAGS) + ["-DDLM_DRAIN_WAITS=1", "-c", s, "-o", o])
    _compile_all(todo, verbose)
    objs = [drain_object(s) if s in DRAIN_SOURCES else os.path.join(HERE, "build", s.replace(".hip", ".o")) for s in SOURCES]
    if force or _stale(DRAIN_LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", DRAIN_LIB] + objs + ["-L/opt/rocm/lib", "-lrccl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return DRAIN_LIB


def build(force=False, verbose=False):
    objs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    todo = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(HERE, "build", src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + HEADERS):
            todo.append([HIPCC] + FILE_FLAGS.get(src, FLAGS) + ["-c", s, "-o", o])
    _compile_all(todo, verbose)
    if force or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-L/opt/rocm/lib", "-lrccl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    if "--drain" in sys.argv:
        build_drain_variant(force="--force" in sys.argv, verbose=True)
