"""In-tree build of the native pieces (no cmake): hipcc for libfdengine.so (gfx950), gcc for the
CPU oracle used by tests and the bench's cpu_baseline leg.

Outputs stay in-tree (git-ignored, but shipped to the GPU box by gpurun):
  realtime-fraud-detection_amd/lib/libfdengine.so
  oracle/build/liboracle.so
"""
from __future__ import annotations

import importlib.util
import os
import shutil
import subprocess
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent
REPO_ROOT = PKG_ROOT.parent
CSRC = PKG_ROOT / "csrc"
LIB_DIR = PKG_ROOT / "lib"
ORACLE_DIR = REPO_ROOT / "oracle"

HIP_SOURCES = ["engine.hip", "score.hip", "forest.hip", "forest_sparse.hip", "shap.hip", "gbdt.hip", "iforest_fit.hip", "ensemble.hip", "ensemble_plan.hip", "blend.hip", "features.hip", "route.hip", "lstm.hip", "mlp.hip", "mlp_fit.hip", "graph.hip", "text.hip", "abtest.hip", "metrics.hip",
               "windows.hip", "snapshot.hip", "ingest.hip", "sink.hip", "model_io.hip", "comm.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage"]
RESOURCES = LIB_DIR / "kernel_resources.json"  # per kernel: VGPRs, AGPRs, scratch, occupancy (the compiler's remarks)


def parse_resource_remarks(text: str) -> dict:
    """hipcc's kernel-resource-usage remarks -> {mangled kernel name: {"vgpr", "agpr", "sgpr", "scratch", "occupancy",
    "lds"}} (tests/test_kernel_budget.py holds the hot kernels to their register budgets)."""
    import re
    out, cur = {}, None
    keys = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (ROCm required to build libfdengine.so)")


def _buildid():
    """fdengine/_buildid.py, loaded by path (the package cannot be imported before its library exists)"""
    spec = importlib.util.spec_from_file_location("fdengine_buildid", Path(__file__).resolve().parent / "_buildid.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stale(out: Path, inputs) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(Path(p).stat().st_mtime > t for p in inputs)


def build_engine(force: bool = False, verbose: bool = True, profile: bool = False) -> Path:
    """One object per translation unit (compiled in parallel), then one link with a generated build-id object.
    Staleness is decided by content, not mtime: the library embeds fd_build_id() (a digest of the HIP sources,
    the csrc headers and include/fdengine.h, plus the flags; fdengine/_buildid.py) and is rebuilt when that
    differs from the tree's; each object is rebuilt when the digest of its source + the headers + flags recorded
    beside it differs. profile=True builds lib/libfdengine_prof.so with the forest and feature kernels'
    phase-cycle instrumentation (-DFD_FOREST_PROFILE; tools/forest_phases.py / tools/feat_phases.py load it
    via FDENGINE_LIB)."""
    from concurrent.futures import ThreadPoolExecutor
    B = _buildid()
    LIB_DIR.mkdir(exist_ok=True)
    obj_dir = LIB_DIR / ("obj_prof" if profile else "obj")
    obj_dir.mkdir(exist_ok=True)
    out = LIB_DIR / ("libfdengine_prof.so" if profile else "libfdengine.so")
    srcs = [CSRC / s for s in HIP_SOURCES if (CSRC / s).exists()]
    headers = sorted(CSRC.glob("*.h")) + [REPO_ROOT / "include" / "fdengine.h"]
    extra = ["-DFD_FOREST_PROFILE"] if profile else []
    compile_flags = [f for f in HIPCC_FLAGS if f != "-shared"] + extra
    want_id = B.id_string(B.source_digest(), compile_flags)
    if not force and B.embedded_id(out) == want_id:
        return out  # (the GPU box gets the library without the objects)

    def obj(src: Path) -> Path:
        o = obj_dir / (src.stem + ".o")
        stamp = o.with_suffix(".o.digest")
        dig = B.digest_files([src, *headers]) + " " + " ".join(compile_flags)
        if force or not o.exists() or not stamp.exists() or stamp.read_text() != dig:
            tmp = o.with_suffix(".o.tmp")
            cmd = [_hipcc(), *compile_flags, f"-I{REPO_ROOT / 'include'}", f"-I{CSRC}", "-c", str(src),
                   "-o", str(tmp)]
            if verbose:
                print("[build]", " ".join(cmd), flush=True)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src.name}:\n{r.stderr[-6000:]}")
            tmp.replace(o)
            import json
            o.with_suffix(".res.json").write_text(json.dumps(parse_resource_remarks(r.stderr), indent=0))
            stamp.write_text(dig)
        return o

    jobs = max(1, min(len(srcs), int(os.environ.get("MAX_JOBS", os.cpu_count() or 4)), 16))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(obj, srcs))
    # the build id: one C function returning the id string (the marker also lets the build read it from the bytes)
    idc = obj_dir / "build_id.c"
    idc.write_text('__attribute__((visibility("default"))) const char* fd_build_id(void) {\n'
                   f'  return "{want_id}";\n}}\n')
    ido = obj_dir / "build_id.o"
    subprocess.run(["gcc", "-O2", "-fPIC", "-c", str(idc), "-o", str(ido)], check=True)
    tmp = out.with_suffix(".so.tmp")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, objs), str(ido), "-o", str(tmp)]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    tmp.replace(out)
    if not profile:
        import json
        res = {}
        for o in objs:
            rj = o.with_suffix(".res.json")
            if rj.exists():
                res.update(json.loads(rj.read_text()))
        RESOURCES.write_text(json.dumps(res, indent=0, sort_keys=True))
    return out


def build_oracle(force: bool = False, verbose: bool = True) -> Path:
    bdir = ORACLE_DIR / "build"
    bdir.mkdir(exist_ok=True)
    out = bdir / "liboracle.so"
    srcs = sorted(ORACLE_DIR.glob("*.c"))
    deps = srcs + sorted(ORACLE_DIR.glob("*.h"))
    if not force and not _stale(out, deps):
        return out
    tmp = out.with_suffix(".so.tmp")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off",
           "-fno-fast-math", *map(str, srcs), "-o", str(tmp), "-lm"]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    tmp.replace(out)
    return out


TEST_NATIVE = REPO_ROOT / "tests" / "native"


def build_test_libs(force: bool = False, verbose: bool = True) -> Path:
    """Test infrastructure: tests/native/rccl_loopback.cpp -> tests/native/build/librccl_loopback.so, the in-process
    loopback of the eight RCCL entry points the sharded step calls (several ranks on one GPU in the GPU tests)."""
    src = TEST_NATIVE / "rccl_loopback.cpp"
    bdir = TEST_NATIVE / "build"
    bdir.mkdir(exist_ok=True)
    out = bdir / "librccl_loopback.so"
    if not force and not _stale(out, [src]):
        return out
    tmp = out.with_suffix(".so.tmp")
    cmd = [_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", str(src), "-o", str(tmp)]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    tmp.replace(out)
    return out


def build_all(force: bool = False, verbose: bool = True) -> None:
    build_engine(force=force, verbose=verbose)
    build_oracle(force=force, verbose=verbose)
    if (TEST_NATIVE / "rccl_loopback.cpp").exists():
        build_test_libs(force=force, verbose=verbose)


if __name__ == "__main__":
    import sys
    build_all(force="--force" in sys.argv)
    if "--profile" in sys.argv:
        build_engine(force="--force" in sys.argv, profile=True)
