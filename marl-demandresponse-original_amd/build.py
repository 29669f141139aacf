"""Build csrc/libmdr_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ("mdr_kernels.hip", "mdr_resident.hip", "mdr_rollout_rows.hip", "mdr_multi.hip", "mdr_persist.hip", "mdr_mailbox.hip", "mdr_control.hip", "mdr_api.hip", "mdr_policy.hip", "mdr_tarmac.hip", "mdr_tarmac_mlp.hip", "mdr_tarmac_mlp_bf16.hip", "mdr_tarmac_grad.hip", "mdr_tarmac_gather.hip", "mdr_ppo_grad.hip", "mdr_ppo_grad_bf16.hip", "mdr_tarmac_ppo_grad.hip", "mdr_optim.hip", "mdr_maddpg_grad.hip", "mdr_mlp_actor.hip", "mdr_mlp_actor_bf16.hip", "mdr_mlp_actor_observe.hip", "mdr_tarmac_critic_grad.hip", "mdr_tarmac_a2c.hip", "mdr_minibatch.hip")
HEADERS = ("mdr_device.h", "mdr_kernels.h", "mdr_step_common.h", "mdr_mailbox.h", "mdr_draw.h", "mdr_bf16_split.h", "mdr_tarmac_mlp.h", "mdr_observe.h", "mdr_grad_reduce.h", "mdr_stream_mlp.h", os.path.join("..", "..", "include", "mdr.h"), os.path.join("..", "..", "include", "mdr_policy.h"))
OUTPUT = os.path.join(CSRC, "libmdr_hip.so")


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libmdr_hip.so)")


def is_stale() -> bool:
    if not os.path.isfile(OUTPUT):
        return True
    built = os.path.getmtime(OUTPUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > built for d in deps)


# -ffp-contract=on: a*b+c fuses only inside one source expression (decided by the front end), never across statements,
# so that every kernel inlining the same house update / reward expression rounds it identically (hipcc's default
# "fast" lets the back end fuse depending on the surrounding code)
FLAGS = ("--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-std=c++17", "-fPIC")
# Extra flags of single translation units, behind FLAGS, in the product library and in every experiment build alike.
# mdr_resident.hip with -fno-slp-vectorize: the resident rollout loop in plain f32 instructions instead of v_pk_*_f32 pairs, the same
# bits (bench.py's dumps are byte-identical).  With one launch per table window it was 4.5 - 4.8 % faster in bench.py, 1.5 and 2.3
# times the run-to-run spread where the project asks for 3 (profiles/r11_README.md section 2), and stayed out; with one launch per
# rollout the loop is nine tenths of the time and the difference is 10 %, 5.5 and 6.1 times the larger spread in two sets of five
# (profiles/r12_README.md section 2).  build_variant(name, source_flags={}) rebuilds the packed arm.
SOURCE_FLAGS = {"mdr_resident.hip": ("-fno-slp-vectorize",)}


def _compile_and_link(out: str, objdir: str, defines=(), source_flags=None, force: bool = False, verbose: bool = False) -> str:
    """One object per source under `objdir` (recompiled when the source or any header is newer), then one link: an edit of one
    kernel file costs that file's compile time, not the library's.  `source_flags` replaces SOURCE_FLAGS (experiment builds)."""
    per_source = SOURCE_FLAGS if source_flags is None else source_flags
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in HEADERS]
    objects, jobs = [], []
    for src in SOURCES:
        path, obj = os.path.join(CSRC, src), os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        objects.append(obj)
        if force or not os.path.isfile(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in [path] + headers):
            cmd = [_hipcc(), *FLAGS, *per_source.get(src, ()), *("-D" + d for d in defines), "-c", path, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    for cmd, proc in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + objects
    if verbose:
        print(" ".join(link))
    subprocess.run(link, check=True, cwd=CSRC)
    return out


def build_variant(name: str, defines=(), source_flags=None, verbose: bool = False) -> str:
    """Experiment build csrc/libmdr_hip_<name>.so with extra -D switches (e.g. MDR_NT_STORES=0 for the cache-control sweep of
    tools/bench_size_sweep.py) and, optionally, other per-source flags than SOURCE_FLAGS (a dict like it; {} = none);
    select it with the MDR_HIP_LIB environment variable.  Never the product library.  Its objects live under csrc/build/<name>/;
    a build with other switches under the same name needs another name."""
    out = os.path.join(CSRC, "libmdr_hip_%s.so" % name)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    if os.path.isfile(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    return _compile_and_link(out, os.path.join(CSRC, "build", name), defines, source_flags, force=True, verbose=verbose)


def build_native(force: bool = False, verbose: bool = False) -> str:
    """csrc/libmdr_hip.so, its objects under csrc/build/."""
    if not force and not is_stale():
        return OUTPUT
    return _compile_and_link(OUTPUT, os.path.join(CSRC, "build"), force=force, verbose=verbose)
