"""The points entry points at the C-ABI boundary, without a device
(include/sdf_abi.h "Points"): the symbols exist, sdf_points and sdf_point_shade
have their layouts, every SDF_E_INVALID_ARG and SDF_E_UNSUPPORTED case is
decided before any device call -- through sdf_validate_points and through
sdf_shade_points, which is handed a stream handle that must never be touched --
and n = 0 is SDF_OK on a machine with no GPU."""
import ctypes as C
import math

import pytest

import lights_ref as LR
import materials_ref as MR
from sdf3d_amd import abi, scenes

OK, INVALID, UNSUPPORTED = abi.SDF_OK, abi.SDF_E_INVALID_ARG, abi.SDF_E_UNSUPPORTED
PTR = 0x1000   # a non-null "device pointer": never dereferenced before a device call
BOGUS_STREAM = C.c_void_p(0xDEAD0000BEEF0)     # never dereferenced: every call here is rejected
NULL = object()


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame(name="C4"):
    return scenes.config(name, 64, 36)


def mats_of(f):
    return MR.palette_for(f) if f.scene.kind == abi.SCENE_PRIMITIVES else [f.material]


def points_of(points=PTR, normals=None, n=1, eye=None, lift=0.0, flags=None, reserved=0):
    p = abi.sdf_points()
    p.points, p.normals, p.n, p.lift, p.reserved = points, normals, n, lift, reserved
    if eye is not None:
        for c in range(3):
            p.eye[c] = eye[c]
    p.flags = (abi.POINTS_EYE if eye is not None else 0) if flags is None else flags
    return p


def shade_of(rgba=PTR, ao=None, shadow=None, material=None, steps=None):
    return abi.sdf_point_shade(rgba, ao, shadow, material, steps)


def call(lib, f, pts=None, out=None, materials=None, lights=None, light_flags=0, scene=True,
         params=True, shade=True):
    """sdf_validate_points (shade False) or sdf_shade_points with the bogus stream."""
    pts = points_of() if pts is None else pts
    out = shade_of() if out is None else out
    lights = [f.light] if lights is None else lights
    larr = (abi.sdf_light * max(len(lights), 1))(*lights)
    marr, nm = MR.marr(mats_of(f) if materials is None else materials)
    head = (C.byref(f.scene) if scene else None, larr if lights else None, len(lights),
            light_flags, marr, nm, C.byref(f.params) if params else None,
            None if pts is NULL else C.byref(pts))
    if not shade:
        return lib.sdf_validate_points(*head)
    return lib.sdf_shade_points(*head, None if out is NULL else C.byref(out), BOGUS_STREAM)


def both(lib, f, **kw):
    a, b = call(lib, f, shade=False, **kw), call(lib, f, shade=True, **kw)
    assert a == b, (a, b)
    return a


def test_symbols_and_layout(lib):
    for name, nargs in (("sdf_validate_points", 8), ("sdf_shade_points", 10)):
        assert hasattr(lib, name), name
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    P, S = abi.sdf_points, abi.sdf_point_shade
    assert C.sizeof(P) == 48 == abi.STRUCT_SIZES["sdf_points"]
    assert C.sizeof(S) == 40 == abi.STRUCT_SIZES["sdf_point_shade"]
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("points", 0), ("normals", 8), ("n", 16), ("eye", 24), ("lift", 36), ("flags", 40),
        ("reserved", 44)]
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("rgba", 0), ("ao", 8), ("shadow", 16), ("material", 24), ("steps", 32)]
    assert abi.POINTS_EYE == 1
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


@pytest.mark.parametrize("cfg", ["REF", "C1", "C2", "C3", "C4", "C5"])
def test_accepts_every_config(lib, cfg):
    f = frame(cfg)
    assert call(lib, f, shade=False) == OK
    assert call(lib, f, points_of(normals=PTR, eye=(1.0, 2.0, -3.0), lift=0.25), shade=False) == OK
    assert call(lib, f, lights=LR.rig(8), light_flags=abi.LIGHTS_COLOR, shade=False) == OK
    # width, height, samples and output_format play no part
    g = f.copy()
    g.params.width, g.params.height, g.params.samples = -5, 0, 3
    g.params.output_format = abi.FORMAT_TILES
    assert call(lib, g, shade=False) == OK


def test_invalid_arguments_before_any_device_call(lib):
    f = frame()
    assert both(lib, f, pts=NULL) == INVALID
    assert call(lib, f, out=NULL) == INVALID
    assert call(lib, f, out=shade_of(rgba=None)) == INVALID                 # every output NULL
    for only in ("rgba", "ao", "shadow", "material", "steps"):               # one is enough
        o = shade_of(rgba=None)
        setattr(o, only, PTR)
        assert call(lib, f, pts=points_of(n=0), out=o) == OK
    for off in (4, 8, 12):                                                   # rgba: 16-byte aligned
        assert call(lib, f, out=shade_of(rgba=PTR + off)) == INVALID, off
        assert call(lib, f, pts=points_of(n=0), out=shade_of(rgba=PTR + off)) == INVALID
        assert call(lib, f, pts=points_of(n=0), out=shade_of(rgba=None, ao=PTR + off)) == OK
    assert both(lib, f, scene=False) == INVALID
    assert both(lib, f, params=False) == INVALID
    assert both(lib, f, pts=points_of(points=None)) == INVALID              # NULL points, n > 0
    assert both(lib, f, pts=points_of(n=-1)) == INVALID
    assert both(lib, f, pts=points_of(n=(1 << 30) + 1)) == INVALID
    assert call(lib, f, pts=points_of(n=1 << 30), shade=False) == OK         # the limit is legal
    for flags in (0x2, 0x3, 0x100, -1, 1 << 30):
        assert both(lib, f, pts=points_of(flags=flags)) == INVALID, flags
    assert both(lib, f, pts=points_of(reserved=1)) == INVALID
    for lift in (math.nan, math.inf, -math.inf, -1e-30, -1.0, 2e15):
        assert both(lib, f, pts=points_of(lift=lift)) == INVALID, lift
    assert call(lib, f, pts=points_of(lift=1e15), shade=False) == OK
    for bad in (math.nan, math.inf, -math.inf, 2e15, -2e15):
        for c in range(3):
            eye = [0.0, 1.0, 2.0]
            eye[c] = bad
            assert both(lib, f, pts=points_of(eye=eye)) == INVALID, (bad, c)
            # without the flag the eye is not read
            assert call(lib, f, pts=points_of(eye=eye, flags=0), shade=False) == OK
    # anything sdf_validate_materials rejects, n = 0 included
    assert both(lib, f, lights=[]) == INVALID
    assert both(lib, f, lights=LR.rig(8) + [f.light]) == INVALID
    assert both(lib, f, light_flags=0x2) == INVALID
    assert both(lib, f, materials=mats_of(f)[:-1]) == INVALID                # one per primitive
    g = f.copy()
    g.params.max_steps = -1
    assert both(lib, g) == INVALID and both(lib, g, pts=points_of(n=0)) == INVALID
    g = f.copy()
    g.scene.prims[2].p[0] = float("nan")
    assert both(lib, g) == INVALID
    g = frame("C5")
    assert both(lib, g, materials=scenes.palette(2)) == INVALID              # a Mandelbulb has one


def test_differing_shininess_stays_unsupported(lib):
    f = frame()
    mats = mats_of(f)
    mats[3].shininess = mats[0].shininess + 1.0
    assert both(lib, f, materials=mats) == UNSUPPORTED
    assert both(lib, f, materials=mats, pts=points_of(n=0)) == UNSUPPORTED


def test_no_points_is_ok_without_a_device(lib):
    f = frame()
    assert call(lib, f, pts=points_of(points=None, n=0)) == OK
    assert call(lib, f, pts=points_of(points=None, normals=None, n=0, eye=(0.0, 1.0, 0.0),
                                      lift=0.5),
                out=shade_of(PTR, PTR, PTR, PTR, PTR)) == OK
    assert call(lib, frame("C5"), pts=points_of(n=0)) == OK
