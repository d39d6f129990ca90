"""Build the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU).

    python -m epipolar_transformers_amd.build [--report]

The .so lands in epipolar_transformers_amd/lib/ (git-ignored, shipped to the
GPU box by gpurun).  -ffp-contract=off is REQUIRED: the geometry in
csrc/epipolar_geometry.h reproduces the reference's float32 roundings op by op
and spells its FMAs explicitly.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
COMMON = ["et_common.h", "epipolar_geometry.h", os.path.join(ROOT, "include", "epipolar_amd.h")]
# translation unit -> the files it includes besides COMMON
UNITS = {
    "et_forward.hip": ["kernels_sample_table.inc", "kernels_pixel_phases.inc", "kernels_forward.inc"],
    "et_forward_general.hip": ["et_wave_reduce.h"],
    "et_forward_tile.hip": ["kernels_tile_order.inc", "kernels_tile_common.inc", "kernels_forward_tile.inc", "kernels_forward_tile_ws.inc",
                            "et_tile_host.h", "et_tile_layout.h", "et_wave_reduce.h", "et_split_f16.h", "et_lds_layout.h"],
    "et_backward.hip": ["kernels_sample_table.inc", "kernels_pixel_phases.inc", "kernels_backward.inc"],
    "et_backward_tile.hip": ["kernels_tile_order.inc", "kernels_tile_common.inc", "kernels_backward_tile.inc", "kernels_backward_det.inc",
                             "et_tile_host.h", "et_tile_layout.h", "et_wave_reduce.h", "et_split_f16.h", "et_lds_layout.h"],
    "et_misc.hip": ["kernels_misc.inc", "et_peaks.h"],
    "et_residual_gemm.hip": ["kernels_residual_gemm.inc", "et_wave_reduce.h"],
    "et_meta.hip": ["kernels_meta.inc", "kernels_residual_gemm.inc", "et_wave_reduce.h"],
    "et_triangulate.hip": ["et_triangulate.h", "et_wave_reduce.h"],
    "et_rpsm.hip": ["et_rpsm.h"],
    "et_metrics.hip": ["et_metrics.h", "et_wave_reduce.h"],
    "et_loss.hip": ["et_loss.h"],
}
LIB = os.path.join(PKG, "lib", "libepipolar_amd.so")
OBJ = os.path.join(PKG, "lib", "obj")
ARCH = "gfx950"
# development builds (never loaded by the product path): `--profile` adds the per-phase cycle counters of the
# warp-specialised forward (scripts/ws_profile.py loads it through EPIPOLAR_AMD_LIB)
PROFILE_LIB = os.path.join(PKG, "lib", "libepipolar_amd_prof.so")


def _path(f):
    return f if os.path.isabs(f) else os.path.join(CSRC, f)


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


_EXTRA = []      # extra defines of a development build (build_profile_library)
# The whole library is compiled WITHOUT SLP vectorisation.  With it the tap arithmetic of the one-block-per-tile forward
# becomes packed-fp32 instructions (v_pk_add_f32 / v_pk_mul_f32 with op_sel), and that kernel then returned wrong attention in
# lanes 48-63 of single pixels whenever blocks running its split-fp16 GEMM shared a SIMD with blocks in the soft-max phase --
# 20 of 20 runs with SLP, 0 of 20 without, nothing else changed (scripts/dev/README.md).  The mechanism is not understood, so
# the flag covers every unit (the other kernels never showed the fault); measured cost: none (step 1.50 vs 1.51 ms,
# backward 2.47 vs 2.45 ms).
_SAFE_FLAGS = ["-fno-slp-vectorize"]
_UNIT_FLAGS = {}     # per-unit extras (none at present)


def _extra_env_flags():
    """ET_EXTRA_HIPCC_FLAGS, minus anything that would undo _SAFE_FLAGS: a flag that re-enables SLP vectorisation (or
    contraction: the geometry must round op by op) is refused loudly rather than producing a library that is wrong
    some of the time."""
    extra = os.environ.get("ET_EXTRA_HIPCC_FLAGS", "").split()
    banned = [f for f in extra if f in ("-fslp-vectorize", "-fvectorize", "-ffast-math", "-Ofast") or
              f.startswith(("-ffp-contract=fast", "-ffp-contract=on")) or (f.startswith("-mllvm") and "slp" in f.lower())]
    if banned or any("slp-vectorizer" in f or "vectorize-slp" in f for f in extra):
        raise RuntimeError("ET_EXTRA_HIPCC_FLAGS carries %s: the library must be built without SLP vectorisation and with "
                           "-ffp-contract=off (build.py: _SAFE_FLAGS, scripts/dev/README.md)" % (banned or extra))
    return extra


def flags():
    return ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"] + _SAFE_FLAGS + \
           ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + _EXTRA + _extra_env_flags()


def _obj(unit):
    return os.path.join(OBJ + ("_dev" if _EXTRA else ""), os.path.splitext(unit)[0] + ".o")


def _stale(unit) -> bool:
    o = _obj(unit)
    if not os.path.exists(o):
        return True
    t = os.path.getmtime(o)
    return any(os.path.getmtime(_path(d)) > t for d in [unit] + UNITS[unit] + COMMON)


def needs_build() -> bool:
    return not os.path.exists(LIB) or any(_stale(u) for u in UNITS) or \
        any(os.path.getmtime(_obj(u)) > os.path.getmtime(LIB) for u in UNITS)


def _compile(unit, report):
    cmd = [hipcc()] + flags() + _UNIT_FLAGS.get(unit, []) + (["-Rpass-analysis=kernel-resource-usage"] if report else []) + \
        ["-c", "-o", _obj(unit), _path(unit)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return unit, proc.returncode, proc.stdout


def build_library(force: bool = False, report: bool = False) -> str:
    """Compile the stale translation units in parallel (one hipcc per unit) and link them into LIB."""
    from concurrent.futures import ThreadPoolExecutor

    os.makedirs(os.path.dirname(_obj("x.hip")), exist_ok=True)
    todo = [u for u in UNITS if force or report or _stale(u)]
    logs = []
    if todo:
        with ThreadPoolExecutor(max_workers=min(len(todo), os.cpu_count() or 1)) as pool:
            for unit, rc, out in pool.map(lambda u: _compile(u, report), todo):
                if rc != 0:
                    sys.stderr.write(out)
                    raise RuntimeError("hipcc failed on %s (exit %d)" % (unit, rc))
                logs.append(out)
    if todo or not os.path.exists(LIB) or any(os.path.getmtime(_obj(u)) > os.path.getmtime(LIB) for u in UNITS):
        cmd = [hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + [_obj(u) for u in UNITS]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout)
            raise RuntimeError("link failed (exit %d)" % proc.returncode)
    if report:
        print(resource_table("\n".join(logs)))
    return LIB


def resource_table(log: str) -> str:
    rows, cur = [], None
    for line in log.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            cur[key.split(" ")[0]] = val
    out = ["%-78s %5s %5s %7s %4s %6s" % ("kernel", "VGPR", "SGPR", "scratch", "occ", "LDS")]
    for r in rows:
        name = subprocess.run(["c++filt", r["name"]], stdout=subprocess.PIPE, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0]
        out.append("%-78s %5s %5s %7s %4s %6s" % (name[:78], r.get("VGPRs"), r.get("TotalSGPRs"),
                                                 r.get("ScratchSize"), r.get("Occupancy"), r.get("LDS")))
    return "\n".join(out)


def build_profile_library(defines=("-DET_WS_PROFILE=2",)) -> str:
    """The same sources with development defines, linked into PROFILE_LIB (objects under lib/obj_dev)."""
    global LIB
    keep = LIB
    _EXTRA[:] = list(defines)
    LIB = PROFILE_LIB
    try:
        os.makedirs(OBJ + "_dev", exist_ok=True)
        return build_library(force=True)
    finally:
        _EXTRA[:] = []
        LIB = keep


if __name__ == "__main__":
    if "--profile" in sys.argv:
        print(build_profile_library(tuple(a for a in sys.argv[1:] if a.startswith(("-D", "-f", "-m"))) or ("-DET_WS_PROFILE=2",)))
    else:
        build_library(force=True, report="--report" in sys.argv)
        print(LIB)
