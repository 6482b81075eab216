"""sdf_mesh_emit_sharp at the C-ABI boundary, without a GPU (include/sdf_abi.h
"Sharp meshes"): symbols and layout, every documented error decided before any
device call (fake pointers, no device), and the NumPy reference's identity."""
import ctypes as C

import numpy as np
import pytest

import cases
import fast_paths as FP
import mesh_sharp_ref as S
from sdf3d_amd import abi, renderer as R, scenes

INVALID, UNSUPPORTED, OK = abi.SDF_E_INVALID_ARG, abi.SDF_E_UNSUPPORTED, abi.SDF_OK
FAKE = C.c_void_p(1 << 20)          # a 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame(name="C4"):
    return scenes.config(name, 64, 36)


def good_grid():
    return R.grid((-1.13, -0.11, -1.02), (0.12, 0.08, 0.11), (19, 11, 17))


def calls(lib, f, g, sharp, ws=FAKE, nbytes=None, out=None):
    """(validate, emit) return codes of one set of arguments."""
    if nbytes is None:
        nbytes = max(int(lib.sdf_mesh_workspace_bytes(C.byref(g))), 0) if g is not None else 0
    o = abi.sdf_mesh_out(FAKE, 10, FAKE, 10, None, None) if out is None else out
    gp = C.byref(g) if g is not None else None
    return (lib.sdf_validate_mesh_sharp(C.byref(f.scene), C.byref(f.params), gp, sharp),
            lib.sdf_mesh_emit_sharp(C.byref(f.scene), C.byref(f.params), gp, sharp, ws, nbytes,
                                    C.byref(o), None))


def test_symbols_and_layout(lib):
    for name, nargs in (("sdf_validate_mesh_sharp", 4), ("sdf_mesh_emit_sharp", 8)):
        assert hasattr(lib, name), name
        assert len(abi.SIGNATURES[name][1]) == nargs
        assert abi.SIGNATURES[name][0] is C.c_int
    assert C.sizeof(abi.sdf_mesh_sharp) == 16 == abi.STRUCT_SIZES["sdf_mesh_sharp"]
    assert [n for n, _ in abi.sdf_mesh_sharp._fields_] == ["refine", "iterations", "flags", "reserved"]
    assert abi.sdf_mesh_sharp.iterations.offset == 4 and abi.sdf_mesh_sharp.reserved.offset == 12
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION
    # the grid got no new flag: what test_mesh_abi.py pins stays invalid
    g = good_grid()
    g.flags = 2
    assert calls(lib, frame(), g, abi.sdf_mesh_sharp(4, 16, 0, 0)) == (INVALID, INVALID)


@pytest.mark.parametrize("sharp", [(-1, 0, 0, 0), (9, 0, 0, 0), (0, -1, 0, 0), (0, 65, 0, 0),
                                   (4, 16, 1, 0), (4, 16, 0, 1), (0, 0, 2, 0), (0, 0, 0, -1)])
def test_bad_sharp_is_refused(lib, sharp):
    assert calls(lib, frame(), good_grid(), abi.sdf_mesh_sharp(*sharp)) == (INVALID, INVALID)
    # a Mandelbulb too: an invalid argument is one before anything is unsupported
    assert calls(lib, frame("C5"), good_grid(), abi.sdf_mesh_sharp(*sharp)) == (INVALID, INVALID)


@pytest.mark.parametrize("sharp", [(8, 64), (4, 16), (1, 0), (0, 1)])
def test_what_sdf_mesh_emit_rejects(lib, sharp):
    sp = abi.sdf_mesh_sharp(*sharp, 0, 0)
    f, g = frame(), good_grid()
    need = int(lib.sdf_mesh_workspace_bytes(C.byref(g)))
    assert calls(lib, f, None, sp) == (INVALID, INVALID)
    assert lib.sdf_validate_mesh_sharp(None, C.byref(f.params), C.byref(g), sp) == INVALID
    assert lib.sdf_validate_mesh_sharp(C.byref(f.scene), None, C.byref(g), sp) == INVALID
    assert calls(lib, f, g, sp, ws=None)[1] == INVALID
    assert calls(lib, f, g, sp, nbytes=need - 1)[1] == INVALID
    assert calls(lib, f, g, sp, ws=C.c_void_p((1 << 20) + 8))[1] == INVALID   # misaligned
    emit = lambda o: lib.sdf_mesh_emit_sharp(C.byref(f.scene), C.byref(f.params), C.byref(g), sp, FAKE,
                                             need, C.byref(o) if o is not None else None, None)
    assert emit(None) == INVALID
    assert emit(abi.sdf_mesh_out(None, 5, FAKE, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, 5, None, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, -1, FAKE, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, 5, FAKE, -1, None, None)) == INVALID
    for bad in ({"n": (1, 0)}, {"cell": (0, 0.0)}, {"reserved": 1}, {"iso": float("nan")}):
        g2 = good_grid()
        for k, v in bad.items():
            if isinstance(v, tuple):
                getattr(g2, k)[v[0]] = v[1]
            else:
                setattr(g2, k, v)
        assert calls(lib, f, g2, sp) == (INVALID, INVALID), bad
    f.params.normal_mode = 7
    assert calls(lib, f, g, sp) == (INVALID, INVALID)
    f = frame()
    f.scene.prims[1].kind = 99
    assert calls(lib, f, g, sp) == (INVALID, INVALID)


def test_mandelbulb_is_unsupported_only_when_sharp(lib):
    f, g = frame("C5"), good_grid()
    zero = abi.sdf_mesh_out(None, 0, None, 0, None, None)
    for sharp in ((4, 16), (1, 0), (0, 1), (8, 64)):
        sp = abi.sdf_mesh_sharp(*sharp, 0, 0)
        assert calls(lib, f, g, sp) == (UNSUPPORTED, UNSUPPORTED)
        assert calls(lib, f, g, sp, out=zero) == (UNSUPPORTED, UNSUPPORTED)
    # NULL and (0, 0) are sdf_mesh_emit, which takes a Mandelbulb
    assert lib.sdf_validate_mesh_sharp(C.byref(f.scene), C.byref(f.params), C.byref(g), None) == OK
    assert calls(lib, f, g, abi.sdf_mesh_sharp(0, 0, 0, 0), out=zero) == (OK, OK)
    assert calls(lib, f, g, None, out=zero) == (OK, OK)


def test_null_and_plain_sharp_are_accepted_where_emit_is(lib):
    g = good_grid()
    for name in scenes.CONFIGS:
        f = scenes.config(name)
        plain = lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g))
        assert plain == OK
        for sp in (None, abi.sdf_mesh_sharp(0, 0, 0, 0)):
            assert lib.sdf_validate_mesh_sharp(C.byref(f.scene), C.byref(f.params), C.byref(g), sp) == OK


def test_zero_capacities_launch_nothing(lib):
    f, g = frame(), good_grid()
    zero = abi.sdf_mesh_out(None, 0, None, 0, None, None)
    for sp in (None, abi.sdf_mesh_sharp(0, 0, 0, 0), abi.sdf_mesh_sharp(4, 16, 0, 0),
               abi.sdf_mesh_sharp(8, 64, 0, 0)):
        assert calls(lib, f, g, sp, out=zero) == (OK, OK)


def test_renderer_sharp_argument():
    assert R.mesh_sharp(None) is None and R.mesh_sharp(False) is None
    sp = R.mesh_sharp(True)
    assert (sp.refine, sp.iterations, sp.flags, sp.reserved) == (4, 16, 0, 0)
    sp = R.mesh_sharp((1, 3))
    assert (sp.refine, sp.iterations, sp.flags, sp.reserved) == (1, 3, 0, 0)


def test_reference_without_a_fit_is_the_plain_mesh():
    """mesh_sharp_ref with refine 0 and no descent step has mesh_ref's vertices bit
    for bit, whatever the normals are; refinement alone moves some of them."""
    f = S.frame_of("BOX-BALL")
    spec = ((-0.5, -0.5, -0.5), (0.1, 0.11, 0.09), (10, 9, 11))
    E = S.edges(f, *spec, 0.0, 0)
    junk = np.random.default_rng(5).normal(size=E["points"].shape).astype(np.float32)
    r = S.mesh(E, junk, 0)
    assert np.array_equal(r["verts"].view(np.uint32), E["plain"]["verts"].view(np.uint32))
    assert r["counts"][0] > 50 and r["clamped"] == 0
    E4 = S.edges(f, *spec, 0.0, 4)
    r4 = S.mesh(E4, junk, 0)
    assert np.array_equal(r4["tris"], r["tris"])
    assert not np.array_equal(r4["verts"].view(np.uint32), r["verts"].view(np.uint32))
    cells = np.asarray(spec[1], dtype=np.float64)
    lo = np.asarray(spec[0]) + r4["cells"] * cells
    assert np.all(r4["verts"] >= lo - 1e-6) and np.all(r4["verts"] <= lo + cells + 1e-6)


def test_box_scenes_share_no_counted_signature():
    """The box scenes are run-time specialised; their sequences are not those of a
    scene whose compilations another test counts, nor a built-in variant's."""
    taken = {cases.signature(build().scene)
             for build in [*cases.COUNTED.values(), *cases.UNCOUNTED.values(), FP.PATHS["C4-carved"]]}
    taken |= {cases.signature(scenes.config(name, 64, 36).scene) for name in ("REF", "C1", "C2", "C3", "C4")}
    box, ball = (cases.signature(S.frame_of(k).scene) for k in ("BOX", "BOX-BALL"))
    assert box != ball and box not in taken and ball not in taken
