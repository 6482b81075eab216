"""Build the HIP C-ABI library ``sdf3d_amd/lib/libsdf3d.so`` for gfx950.

Explicit ``hipcc`` invocations (no JIT, no torch extension cache) so the built
library lives in-tree and travels to the GPU box with the repository snapshot.

Translation units:
  render_exact.hip  -- render kernel, -ffp-contract=off, IEEE div/sqrt
  render_fast.hip   -- render kernel, FMA contraction, hardware sqrt/rcp
  render_{exact,fast}_bulb.hip -- the Mandelbulb scene's kernels of each
                       precision, built with an ILP scheduler
                       (each of the four: the kernels, render_kernel.inc, and
                       behind them the unit's host launchers, render_launch.inc,
                       exported as one table, host_api.h RenderUnit)
  deinterleave.hip  -- multi-device row-block scatter
  tiles.hip         -- TILES wire format: offset scan, compaction, decode
  mesh.hip          -- the offset scan between sdf_mesh_count and sdf_mesh_emit
  sdf_abi.cpp       -- the extern "C" entry points of include/sdf_abi.h
  jit.cpp           -- run-time scene specialisation (hipRTC)
  driver.cpp        -- the native multi-device frame driver (RCCL, loaded at
                       run time)
  multi.cpp         -- single-process multi-device frames (sdf_render_multi)

Run ``python -m sdf3d_amd.build`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
OBJ = PKG / "build"
LIB_DIR = PKG / "lib"
LIB = LIB_DIR / "libsdf3d.so"


def _abi_version() -> int:
    import re
    m = re.search(r"#define SDF_ABI_VERSION (\d+)", (ROOT / "include" / "sdf_abi.h").read_text())
    return int(m.group(1))


SONAME = f"libsdf3d.so.{_abi_version()}"
ARCH = os.environ.get("SDF3D_ARCH", "gfx950")

COMMON = ["-O3", "-fPIC", "-std=c++17", "-Wall", f"--offload-arch={ARCH}"]
UNITS = [
    # -fno-slp-vectorize: on gfx950 v_pk_*_f32 issue at twice the cycles of
    # their scalar forms (tools/valu_rates.hip) and cannot take abs modifiers,
    # so SLP packing only adds shuffles and v_and masks (and SGPRs)
    ("render_exact.hip", ["-ffp-contract=off", "-fno-slp-vectorize"]),
    # fast-honor-pragmas: FMA contraction everywhere except where a pragma
    # pins an operation sequence (shade.h: the colour must come out the same
    # in the render kernels and the TILES decoder); plain =fast would fuse
    # across the pragma
    ("render_fast.hip", ["-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize"]),
    # the Mandelbulb scene's kernels, scheduled for ILP (its 12-iteration map
    # is one long dependent chain per lane): C5 fast ~1 % faster than the
    # default scheduler, which the CSG8 kernels keep (they gain nothing, or
    # lose up to 7 %; profiles/r04_ab_sched_strategy.json).  The exact one
    # with the iterative ILP scheduler since round 6 (0.1-0.9 % faster than
    # max-ilp at 7 waves/SIMD, profiles/r06_ab_bulb_sched_C5.json), and at 8
    # waves/SIMD since the library log and pow fall-backs became calls
    # (cr_math.h library_log: their fp64 constants no longer occupy VGPRs,
    # 66 -> 53 at 7 waves, 8 waves without scratch): 1.2-2.1 % faster than 7
    # (profiles/r06_ab_cold_calls.json)
    ("render_fast_bulb.hip", ["-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize",
                              "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    ("render_exact_bulb.hip", ["-ffp-contract=off", "-fno-slp-vectorize",
                               "-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]),
    ("deinterleave.hip", []),
    ("heatmap.hip", []),
    ("tiles.hip", ["-ffp-contract=fast-honor-pragmas"]),
    ("mesh.hip", []),
    ("sdf_abi.cpp", ["-ffp-contract=off", "-x", "hip"]),
    ("jit.cpp", ["-x", "hip"]),
    ("driver.cpp", ["-x", "hip"]),
    ("multi.cpp", ["-x", "hip"]),
    ("frames.cpp", ["-ffp-contract=off", "-x", "hip"]),
]
# The device sources, in the order render_kernel.inc takes them: what the
# built-in render kernels of one precision are made of (kernel_id: kernel
# sources alone, no host launcher), what hipRTC is given for a run-time
# specialisation (rtc_sources.inc) and, with the host-only headers, what makes
# an object stale.  An entry is (include name, path); the name is the path
# from csrc/, as the files include one another.  The one list of them.
KERNEL_SOURCES = [(n, Path(os.path.normpath(CSRC / n))) for n in (
    "render_kernel.inc", "kernel_args.h", "../../include/sdf_abi.h", "wave_bits.h", "shade.h",
    "cr_math.h", "kmath.inc", "prims.inc", "store.inc", "scenes.inc", "trace.inc",
    "pixel_paths.inc", "render_entry.inc", "query_kernel.inc", "grad_kernel.inc",
    "mesh_kernel.inc", "measure_kernel.inc", "rays_kernel.inc", "points_kernel.inc", "jit_entry.inc")]
HEADERS = [p for _, p in KERNEL_SOURCES] + [CSRC / "host_api.h", CSRC / "render_launch.inc",
                                            CSRC / "turbo_lut.inc"]


def write_rtc_sources() -> Path:
    """The device sources as the two columns hiprtcCreateProgram takes (include
    names, texts) and their count, embedded into the library (jit.cpp)."""
    out = OBJ / "rtc_sources.inc"
    if _stale(out, [*(p for _, p in KERNEL_SOURCES), Path(__file__)]):
        texts = [p.read_text() for _, p in KERNEL_SOURCES]
        assert not any(')SDF3D"' in t for t in texts)
        out.write_text(
            "// generated by sdf3d_amd/build.py (KERNEL_SOURCES) -- kernel sources for hipRTC\n"
            f"static const int kRtcCount = {len(texts)};\n"
            "static const char* kRtcNames[] = {\n"
            + "".join(f'    "{n}",\n' for n, _ in KERNEL_SOURCES) + "};\n"
            "static const char* kRtcTexts[] = {\n"
            + "".join(f'    R"SDF3D({t})SDF3D",\n' for t in texts) + "};\n")
    return out


def _compiler_version() -> str:
    try:
        return subprocess.run([_hipcc(), "--version"], capture_output=True, text=True,
                              check=True).stdout
    except Exception:  # noqa: BLE001 - the id then covers sources and flags only
        return "unknown"


# the render translation units of each precision (kernel_id)
PRECISION_UNITS = {"render_exact.hip": ("render_exact.hip", "render_exact_bulb.hip"),
                   "render_fast.hip": ("render_fast.hip", "render_fast_bulb.hip")}


def kernel_id(unit: str, compiler: str | None = None) -> str:
    """Build identity of a precision's render kernels (unit render_fast.hip /
    render_exact.hip, with its Mandelbulb unit): SHA-256 over their sources,
    compile flags and the compiler version, 16 hex digits (sdf_abi.h
    sdf_kernel_id).  Paths and timestamps do not enter, so a rebuild elsewhere
    gets the same id."""
    import hashlib
    h = hashlib.sha256()
    units = PRECISION_UNITS.get(unit, (unit,))
    for u in units:
        h.update(u.encode() + b"\0" + (CSRC / u).read_bytes() + b"\0")
    for name, p in KERNEL_SOURCES:
        h.update(name.encode() + b"\0" + p.read_bytes() + b"\0")
    for u in units:
        h.update(" ".join([*COMMON, *dict(UNITS)[u]]).encode() + b"\0")
    h.update((compiler if compiler is not None else _compiler_version()).encode())
    return h.hexdigest()[:16]


def write_kernel_ids() -> Path:
    out = OBJ / "kernel_id.inc"
    comp = _compiler_version()
    text = ("// generated by sdf3d_amd/build.py (kernel_id) -- sdf_kernel_id()\n"
            f'#define SDF_KERNEL_ID_EXACT "{kernel_id("render_exact.hip", comp)}"\n'
            f'#define SDF_KERNEL_ID_FAST "{kernel_id("render_fast.hip", comp)}"\n')
    if not out.exists() or out.read_text() != text:
        out.write_text(text)
    return out


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(exe).exists():
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(str(c) for c in cmd), flush=True)
    subprocess.run([str(c) for c in cmd], check=True)


def build_library(force: bool = False, verbose: bool = True) -> Path:
    hipcc = _hipcc()
    OBJ.mkdir(parents=True, exist_ok=True)
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    objs = []
    rtc = write_rtc_sources()
    kid = write_kernel_ids()
    for src, extra in UNITS:
        s = CSRC / src
        o = OBJ / (s.stem + ".o")
        objs.append(o)
        deps = [s, *HEADERS, Path(__file__)] + ([rtc] if src == "jit.cpp" else []) + (
            [kid] if src == "sdf_abi.cpp" else [])
        if force or _stale(o, deps):
            _run([hipcc, *COMMON, *extra, "-I", OBJ, "-c", s, "-o", o], verbose)
    if force or _stale(LIB, objs):
        tmp = LIB.with_suffix(".so.tmp")
        _run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *objs, "-lhiprtc",
              "-ldl", f"-Wl,-soname,{SONAME}"], verbose)
        os.replace(tmp, LIB)
    # the soname the C++ host links against (bumped with SDF_ABI_VERSION)
    link = LIB_DIR / SONAME
    if not (link.is_symlink() and os.readlink(link) == LIB.name):
        if link.exists() or link.is_symlink():
            link.unlink()
        link.symlink_to(LIB.name)
    return LIB


STATS_LIB = LIB_DIR / "libsdf3d_stats.so"


def build_stats_library(force: bool = False, verbose: bool = True) -> Path:
    """Debug variant of the library whose fast-precision kernel counts
    wave-level culling / evaluation events (render_kernel.inc SDF_STATS;
    read with sdf_debug_stats, tools/kernel_stats.py).  Not used by the
    product path."""
    hipcc = _hipcc()
    odir = OBJ / "stats"
    odir.mkdir(parents=True, exist_ok=True)
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    write_rtc_sources()
    write_kernel_ids()
    objs = []
    for src, extra in UNITS:
        s = CSRC / src
        o = odir / (s.stem + ".o")
        objs.append(o)
        flags = [*extra, "-DSDF_STATS=1"] if src == "render_fast.hip" else extra
        if force or _stale(o, [s, *HEADERS, Path(__file__)]):
            _run([hipcc, *COMMON, *flags, "-I", OBJ, "-c", s, "-o", o], verbose)
    if force or _stale(STATS_LIB, objs):
        _run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", STATS_LIB, *objs,
              "-lhiprtc", "-ldl"], verbose)
    return STATS_LIB


BIN_DIR = PKG / "bin"
EXAMPLE = ROOT / "examples" / "sdf_main.cpp"


def build_example(force: bool = False, verbose: bool = True) -> Path:
    """The headless C++ host program over include/sdf3d.hpp (links libsdf3d.so)."""
    BIN_DIR.mkdir(parents=True, exist_ok=True)
    exe = BIN_DIR / "sdf_main"
    deps = [EXAMPLE, ROOT / "include" / "sdf3d.hpp", ROOT / "include" / "sdf_abi.h", LIB]
    if force or _stale(exe, deps):
        _run([_hipcc(), "-O2", "-std=c++17", f"--offload-arch={ARCH}", "-I", ROOT / "include",
              EXAMPLE, "-L", LIB_DIR, "-lsdf3d", "-Wl,-rpath,$ORIGIN/../lib", "-o", exe], verbose)
    return exe


SHMCOMM_SRC = ROOT / "tests" / "shmcomm" / "shmcomm.cpp"
SHMCOMM_LIB = ROOT / "tests" / "shmcomm" / "libshmcomm.so"


def build_shmcomm(force: bool = False, verbose: bool = True) -> Path:
    """TEST INFRASTRUCTURE: the stand-in for the RCCL symbols the native driver
    loads (tests/shmcomm/shmcomm.cpp), so its multi-rank sequence runs with
    several ranks on one GPU.  Never linked into libsdf3d.so."""
    if force or _stale(SHMCOMM_LIB, [SHMCOMM_SRC, Path(__file__)]):
        _run([_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", SHMCOMM_SRC,
              "-o", SHMCOMM_LIB, "-lrt"], verbose)
    return SHMCOMM_LIB


CRMATH_SRC = ROOT / "tests" / "crmath" / "crmath_check.hip"
CRMATH_EXE = ROOT / "tests" / "crmath" / "crmath_check"


def build_crmath_check(force: bool = False, verbose: bool = True) -> Path:
    """TEST INFRASTRUCTURE: the exhaustive GPU check of the exact kernel's
    correctly rounded sqrt / log / smooth-min division (csrc/cr_math.h), with
    the exact translation unit's floating-point flags.  Never linked into
    libsdf3d.so."""
    flags = dict(UNITS)["render_exact.hip"]
    if force or _stale(CRMATH_EXE, [CRMATH_SRC, CSRC / "cr_math.h", CSRC / "shade.h",
                                    Path(__file__)]):
        _run([_hipcc(), *COMMON, *flags, CRMATH_SRC, "-o", CRMATH_EXE], verbose)
    return CRMATH_EXE


def build_oracle(verbose: bool = True) -> Path:
    """Compile the CPU oracle (test infrastructure) with its own Makefile."""
    _run(["make", "-s", "-C", ROOT / "oracle"], verbose)
    return ROOT / "oracle" / "build" / "liboracle.so"


# TEST INFRASTRUCTURE: references over the CPU oracle (tests/*_ref.c, each
# includes oracle/sdf_oracle.c), built with the oracle's floating-point flags
# (oracle/Makefile: no contraction, no fast-math).  Never linked into
# libsdf3d.so.
REF_FLAGS = ["-O3", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno",
             "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-function", "-shared"]


def _build_ref(name: str, force: bool, verbose: bool, over_materials: bool = True) -> Path:
    """tests/build/lib<name>_ref.so from tests/<name>_ref.c; over_materials:
    linked against the material fold's reference beside it (found through
    $ORIGIN)."""
    src = ROOT / "tests" / f"{name}_ref.c"
    lib = ROOT / "tests" / "build" / f"lib{name}_ref.so"
    deps = [src, ROOT / "oracle" / "sdf_oracle.c", ROOT / "oracle" / "oracle_core.h",
            ROOT / "include" / "sdf_abi.h"]
    link = []
    if over_materials:
        deps.append(build_materials_ref(force=force, verbose=verbose))
        link = ["-L", lib.parent, "-lmaterials_ref", "-Wl,-rpath,$ORIGIN"]
    if force or _stale(lib, deps):
        lib.parent.mkdir(parents=True, exist_ok=True)
        tmp = lib.with_suffix(".so.tmp")
        _run([os.environ.get("CC", "gcc"), *REF_FLAGS, "-o", tmp, src, *link, "-lm"], verbose)
        os.replace(tmp, lib)
    return lib


def build_materials_ref(force: bool = False, verbose: bool = True) -> Path:
    """The material fold's reference."""
    return _build_ref("materials", force, verbose, over_materials=False)


def build_reflect_ref(force: bool = False, verbose: bool = True) -> Path:
    """The reference of mirror reflections."""
    return _build_ref("reflect", force, verbose)


def build_points_ref(force: bool = False, verbose: bool = True) -> Path:
    """The reference of shading at caller-supplied points."""
    return _build_ref("points", force, verbose)


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    build_example(force="--force" in sys.argv)
    build_shmcomm(force="--force" in sys.argv)
    build_crmath_check(force="--force" in sys.argv)
    build_oracle()
    build_materials_ref(force="--force" in sys.argv)
    build_reflect_ref(force="--force" in sys.argv)
    build_points_ref(force="--force" in sys.argv)
