"""The device sources as hipRTC gets them: the manifest (sdf3d_amd/build.py
KERNEL_SOURCES) is closed, and a run-time specialised unit of every family
compiles from exactly its texts.  No GPU: libhiprtc compiles without one.

A unit is what jit.cpp jit_source writes -- definitions and one #include, by the
contract at the top of csrc/jit_entry.inc -- for the signature (0, 8, 17): a
sphere, a smooth-union box and a capsule, the smallest list that instantiates
every branch of FixedScene (a cullable suffix, a smooth operator, three
primitives).  A source missing from the manifest would not fail a GPU test: the
launchers fall back to the generic kernel, which gives the same bits."""
import ctypes as C
import re
from pathlib import Path

import pytest

from sdf3d_amd import build

CSRC = build.CSRC
NAMES = [n for n, _ in build.KERNEL_SOURCES]
TEXTS = {n: p.read_text() for n, p in build.KERNEL_SOURCES}
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
HOST_ONLY = {"host_api.h", "render_launch.inc", "turbo_lut.inc"}
SIGNATURE = (0, 8, 17)
FLAGS = ("TILES", "STEPS", "SSAA", "LIGHTS", "MATERIALS", "REFLECT", "ENV")

# (family, the macro's value, the flags that are on)
UNITS = [("render", "", ()),
         ("render", "", ("TILES", "STEPS")),
         ("render", "", ("STEPS", "SSAA", "LIGHTS", "MATERIALS", "REFLECT", "ENV")),
         ("query", "1", ()),
         ("rays", "", ("STEPS", "ENV")),
         ("mesh", "0", ()),          # mesh_count
         ("mesh", "2", ()),          # mesh_emit_sharp
         ("points", "", ("STEPS",))]


def unit_source(exact: bool, family: str, value: str, on) -> str:
    lines = [f"#define SDF_EXACT {int(exact)}",
             "#define SDF_JIT_SIGNATURE " + ", ".join(map(str, SIGNATURE)),
             f"#define SDF_JIT_{family.upper()} {value}"]
    lines += [f"#define SDF_JIT_{f} {'true' if f in on else 'false'}" for f in FLAGS]
    return "\n".join(lines) + '\n#include "render_kernel.inc"\n'


@pytest.fixture(scope="module")
def hiprtc():
    rocm = Path(build._hipcc()).resolve().parent.parent
    lib = C.CDLL(str(rocm / "lib" / "libhiprtc.so"))
    lib.hiprtcCreateProgram.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_int,
                                        C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    lib.hiprtcCompileProgram.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
    lib.hiprtcGetCodeSize.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.hiprtcGetCode.argtypes = [C.c_void_p, C.c_char_p]
    lib.hiprtcGetProgramLogSize.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.hiprtcGetProgramLog.argtypes = [C.c_void_p, C.c_char_p]
    lib.hiprtcDestroyProgram.argtypes = [C.POINTER(C.c_void_p)]
    return lib


def compile_unit(lib, source: str, exact: bool, names=NAMES):
    """(code object or None, log): `source` compiled for gfx950 with the texts
    of `names` under their names and jit.cpp's five options."""
    texts = (C.c_char_p * len(names))(*(TEXTS[n].encode() for n in names))
    incs = (C.c_char_p * len(names))(*(n.encode() for n in names))
    prog = C.c_void_p()
    assert lib.hiprtcCreateProgram(C.byref(prog), source.encode(), b"sdf_jit.hip", len(names),
                                   texts, incs) == 0
    opts = [b"--offload-arch=gfx950", b"-O3", b"-std=c++17", b"-fno-slp-vectorize",
            b"-ffp-contract=off" if exact else b"-ffp-contract=fast-honor-pragmas"]
    ok = lib.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts)) == 0
    n = C.c_size_t()
    lib.hiprtcGetProgramLogSize(prog, C.byref(n))
    log = C.create_string_buffer(max(n.value, 1))
    lib.hiprtcGetProgramLog(prog, log)
    code = None
    if ok:
        assert lib.hiprtcGetCodeSize(prog, C.byref(n)) == 0 and n.value > 0
        buf = C.create_string_buffer(n.value)
        assert lib.hiprtcGetCode(prog, buf) == 0
        code = buf.raw
    lib.hiprtcDestroyProgram(C.byref(prog))
    return code, log.value.decode(errors="replace")


def test_manifest_is_closed():
    """Every #include "..." of a manifest file names a manifest entry (system
    headers are <...> includes behind #ifndef __HIPCC_RTC__)."""
    assert len(set(NAMES)) == len(NAMES)
    for name, text in TEXTS.items():
        for inc in INCLUDE.findall(text):
            assert inc in NAMES, f'{name} includes "{inc}", which is not in KERNEL_SOURCES'


def test_manifest_covers_the_render_units():
    """Every .inc and .h of csrc/ that a render unit includes, directly or
    through another, is in the manifest, the host-only three excepted."""
    seen, todo = set(), [CSRC / u for u in build.PRECISION_UNITS["render_exact.hip"]
                         + build.PRECISION_UNITS["render_fast.hip"]]
    while todo:
        f = todo.pop()
        for inc in INCLUDE.findall(f.read_text()):
            p = (CSRC / inc).resolve()
            if p.parent == CSRC and p.exists() and p not in seen:
                seen.add(p)
                todo.append(p)
    assert CSRC / "trace.inc" in seen   # the walk does follow the layers
    paths = {p.resolve() for _, p in build.KERNEL_SOURCES}
    missing = sorted(p.name for p in seen if p.name not in HOST_ONLY and p not in paths)
    assert not missing, f"included by a render unit but not in KERNEL_SOURCES: {missing}"


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("family,value,on", UNITS,
                         ids=[f"{f}{v}-{'+'.join(on) or 'plain'}" for f, v, on in UNITS])
def test_unit_compiles(hiprtc, family, value, on, exact):
    code, log = compile_unit(hiprtc, unit_source(exact, family, value, on), exact)
    assert code is not None, log
    assert f"sdf_jit_{family}".encode() in code


def test_unit_needs_every_layer(hiprtc):
    """The same compile with one layer file left out of the table fails."""
    source = unit_source(False, "query", "1", ())
    code, log = compile_unit(hiprtc, source, False, [n for n in NAMES if n != "trace.inc"])
    assert code is None and "trace.inc" in log, log
