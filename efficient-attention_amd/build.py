#!/usr/bin/env python3
"""Build libea_hip.so (and the hardware probe) for gfx950 with hipcc, in-tree.

    python efficient-attention_amd/build.py [--force]

hipcc cross-compiles without a GPU; the resulting lib/libea_hip.so travels with the repo
snapshot to the GPU box (it is git-ignored but not gpurun-ignored)."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-mfma-vgpr-form: MFMA accumulators stay in the architectural VGPRs.  Left to its heuristics hipcc 7.2 parks them
# in AGPRs whenever a loop also touches them with VALU code (online-softmax rescale, P / dS products) and pays a
# v_accvgpr_read/write pair per register per iteration: 17 k such moves in ea_softmax.hip, 14 k in ea_window_bwd.hip.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-I" + INCLUDE, "-I" + CSRC]

LIB_SOURCES = ["ea_capi.hip", "ea_window_fwd.hip", "ea_window_bwd.hip", "ea_eva_landmark.hip",
               "ea_lara_x.hip", "ea_lara_y.hip", "ea_lara_f.hip", "ea_softmax.hip",
               "ea_lara_merge.hip", "ea_proj.hip", "ea_lara_segment.hip",
               "ea_rows_mlp.hip", "ea_wgrad.hip", "ea_linear.hip", "ea_lmk2.hip", "ea_scatter.hip", "ea_proj_rs.hip",
               "ea_performer_f32.hip", "ea_fold.hip", "ea_lara_seglin.hip", "ea_layernorm.hip", "ea_dgrad_rs.hip", "ea_f32_attn.hip",
               "ea_kernelized.hip", "ea_ceva_decode.hip", "ea_ceva_decode_linear.hip", "ea_ceva_decode_vocab.hip", "ea_lara_xp.hip",
               "ea_vocab_score.hip", "ea_adaptive_score.hip", "ea_adaptive_pick.hip", "ea_vocab_nll.hip", "ea_adaptive_nll.hip",
               "ea_linear_rs192.hip"]


def _cuid(src):
    """hipcc derives a translation unit's compilation-unit id (part of its fat-binary symbol names) from a hash that includes
    the OUTPUT path: the same source compiled to two places gives two different objects.  A fixed id per source makes the
    library a pure function of the sources -- its sha256 is what profiles/pmc_*.json are stamped with."""
    return "-cuid=" + os.path.splitext(src)[0]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: %s\n%s" % (" ".join(cmd), r.stdout))
    return r.stdout


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    headers = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h"))
    objs, jobs = [], []
    for src in LIB_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        if force or _newer(o, [s] + headers):
            if verbose:
                print("hipcc -c", src, flush=True)
            jobs.append([HIPCC] + FLAGS + [_cuid(src), "-c", s, "-o", o])
        objs.append(o)
    if jobs:                                             # translation units are independent: compile in parallel
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as pool:
            list(pool.map(_run, jobs))
    lib = os.path.join(LIBDIR, "libea_hip.so")
    if force or _newer(lib, objs):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib])
    probe_src = os.path.join(CSRC, "probe_primitives.hip")
    probe = os.path.join(LIBDIR, "probe_primitives")
    if force or _newer(probe, [probe_src]):
        _run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", probe_src, "-o", probe])
    return lib


def build_from_scratch(verbose=False):
    """Every translation unit compiled afresh into a scratch directory and linked there (ignores the objects and the library
    that travelled with the tree); the in-tree library is replaced only when the fresh one differs byte for byte (hipcc is
    deterministic here: same sources -> same sha256, which the committed counter summaries under profiles/ are stamped
    with).  ~1 minute on the build container.  -> (path of the in-tree library, "identical" | "replaced")."""
    import hashlib
    import shutil
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(LIBDIR, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="ea_build_")
    try:
        jobs, objs = [], []
        for src in LIB_SOURCES:
            o = os.path.join(tmp, src.replace(".hip", ".o"))
            jobs.append([HIPCC] + FLAGS + [_cuid(src), "-c", os.path.join(CSRC, src), "-o", o])
            objs.append(o)
            if verbose:
                print("hipcc -c", src, flush=True)
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as pool:
            list(pool.map(_run, jobs))
        fresh = os.path.join(tmp, "libea_hip.so")
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", fresh])
        lib = os.path.join(LIBDIR, "libea_hip.so")

        def sha(path):
            return hashlib.sha256(open(path, "rb").read()).hexdigest()
        if os.path.exists(lib) and sha(lib) == sha(fresh):
            verdict = "identical"
        else:
            for o in objs:
                shutil.copy2(o, os.path.join(LIBDIR, os.path.basename(o)))
            shutil.copy2(fresh, lib)
            verdict = "replaced"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    build()                      # the probe binary (and nothing else: objects and library are current now)
    return lib, verdict


if __name__ == "__main__":
    if "--from-scratch" in sys.argv:
        print(build_from_scratch(verbose=True))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
