"""C-ABI tests of the mirror-reflection entry points that need no GPU
(include/sdf_abi.h "Reflections"): sdf_validate_reflect and sdf_render_reflect
are exported with the table's signatures and reject what the header lists with
the documented codes before any device call -- the render entry is handed a
stream handle that must never be touched -- and the ABI version and the struct
sizes stay as they were."""
import ctypes as C
import inspect
import math

import pytest

import lights_ref as LR
import materials_ref as MR
import reflect_ref as RR
from sdf3d_amd import abi, renderer as R, scenes

BOGUS_STREAM = C.c_void_p(0xDEAD0000BEEF0)     # never dereferenced: every call here is rejected
NULL = object()


def lib():
    return abi.load_library()


def _args(f, materials, reflect, lights, flags):
    lights = [f.light] if lights is None else lights
    larr = (abi.sdf_light * len(lights))(*lights)
    marr, n = MR.marr(materials)
    ref = None if reflect is NULL else C.byref(reflect)
    return (C.byref(f.scene), C.byref(f.camera), larr, len(lights), flags, marr, n, ref,
            C.byref(f.params))


def validate(f, materials, reflect, lights=None, flags=0, t=None):
    return lib().sdf_validate_reflect(*_args(f, materials, reflect, lights, flags),
                                      C.byref(t) if t is not None else None)


def render(f, materials, reflect, lights=None, flags=0):
    """sdf_render_reflect with null buffers and the bogus stream."""
    return lib().sdf_render_reflect(*_args(f, materials, reflect, lights, flags), None, None,
                                    None, None, BOGUS_STREAM)


def both(f, materials, reflect, **kw):
    a, b = validate(f, materials, reflect, **kw), render(f, materials, reflect, **kw)
    assert a == b, (a, b)
    return a


def frame(cfg="C3"):
    return scenes.config(cfg, *LR.SHAPE)


def test_exports_signatures_and_sizes():
    for name, nargs in (("sdf_validate_reflect", 10), ("sdf_render_reflect", 14)):
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert args[7] == C.POINTER(abi.sdf_reflect)
        assert hasattr(lib(), name)
    assert C.sizeof(abi.sdf_reflect) == 16 == abi.STRUCT_SIZES["sdf_reflect"]
    assert [n for n, _ in abi.sdf_reflect._fields_] == ["bounces", "strength", "layer", "flags"]
    assert abi.MAX_BOUNCES == 4 and abi.REFLECT_WEIGHT == 1
    assert lib().sdf_abi_version() == 12 == abi.SDF_ABI_VERSION
    assert C.sizeof(abi.sdf_params) == 80 and C.sizeof(abi.sdf_material) == 40


@pytest.mark.parametrize("cfg", ["REF", "C1", "C2", "C3", "C4", "C5"])
def test_accepts_every_bounce_count_and_layer(cfg):
    f = frame(cfg)
    mats = MR.palette_for(f) if cfg != "C5" else [f.material]
    for b in range(abi.MAX_BOUNCES + 1):
        for layer in range(-1, b + 1):
            assert validate(f, mats, RR.reflect(b, 0.75, layer)) == abi.SDF_OK, (b, layer)
            if layer >= 0:
                assert validate(f, mats, RR.reflect(b, 0.75, layer, abi.REFLECT_WEIGHT)) == abi.SDF_OK
    assert validate(f, mats, RR.reflect(3, -2.0), LR.rig(8), abi.LIGHTS_COLOR) == abi.SDF_OK


def test_null_reflect():
    f = frame()
    assert both(f, scenes.palette(8), NULL) == abi.SDF_E_INVALID_ARG


def test_bounces_layer_flags_and_strength():
    f, pal = frame(), scenes.palette(8)
    for b in (-1, 5, 1 << 30, -(1 << 31)):
        assert both(f, pal, RR.reflect(b, 1.0)) == abi.SDF_E_INVALID_ARG, b
    for b, layer in ((0, 1), (2, 3), (4, 5), (2, -2), (0, -2)):
        assert both(f, pal, RR.reflect(b, 1.0, layer)) == abi.SDF_E_INVALID_ARG, (b, layer)
    for flags in (0x2, 0x3, 0x100, -1):
        assert both(f, pal, RR.reflect(2, 1.0, 1, flags)) == abi.SDF_E_INVALID_ARG, flags
    # the weight flag names a layer's plane: not the composite's
    assert both(f, pal, RR.reflect(2, 1.0, -1, abi.REFLECT_WEIGHT)) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, RR.reflect(0, 1.0, -1, abi.REFLECT_WEIGHT)) == abi.SDF_E_INVALID_ARG
    for s in (math.nan, math.inf, -math.inf):
        assert both(f, pal, RR.reflect(2, s)) == abi.SDF_E_INVALID_ARG, s
        assert both(f, pal, RR.reflect(0, s)) == abi.SDF_E_INVALID_ARG, s
    for s in (0.0, -0.0, -3.0, 1e30, 1e-40):
        assert validate(f, pal, RR.reflect(2, s)) == abi.SDF_OK, s


@pytest.mark.parametrize("field", ["amb", "dif", "ref"])
def test_material_components_are_finite_when_a_ray_is_reflected(field):
    f = frame()
    for bad in (math.nan, math.inf):
        pal = scenes.palette(8)
        getattr(pal[5], field)[1] = bad
        assert both(f, pal, RR.reflect(1, 1.0)) == abi.SDF_E_INVALID_ARG
        assert both(f, pal, RR.reflect(4, 1.0, 2)) == abi.SDF_E_INVALID_ARG
        # without a bounce the call is sdf_render_materials, which takes any value
        assert validate(f, pal, RR.reflect(0, 1.0)) == abi.SDF_OK
    g = frame("C5")
    m = type(g.material).from_buffer_copy(g.material)
    getattr(m, field)[0] = math.nan
    assert both(g, [m], RR.reflect(2, 1.0)) == abi.SDF_E_INVALID_ARG


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_term_streams_carry_one_layer(fmt):
    f = frame()
    f.params.output_format = fmt
    same = [type(f.material).from_buffer_copy(f.material) for _ in range(8)]
    # no bounce: sdf_validate_materials's answer, served for one material
    assert validate(f, same, RR.reflect(0, 1.0)) == abi.SDF_OK
    assert validate(f, same, RR.reflect(0, 1.0, 0)) == abi.SDF_OK
    assert both(f, scenes.palette(8), RR.reflect(0, 1.0)) == abi.SDF_E_UNSUPPORTED
    for b in (1, 4):
        assert both(f, same, RR.reflect(b, 1.0)) == abi.SDF_E_UNSUPPORTED
        assert both(f, same, RR.reflect(b, 1.0, 0)) == abi.SDF_E_UNSUPPORTED
    assert both(f, same, RR.reflect(0, 1.0, 0, abi.REFLECT_WEIGHT)) == abi.SDF_E_UNSUPPORTED
    g = frame("C5")
    g.params.output_format = fmt
    assert validate(g, [g.material], RR.reflect(0, 1.0)) == abi.SDF_OK
    assert both(g, [g.material], RR.reflect(1, 1.0)) == abi.SDF_E_UNSUPPORTED
    for other in (abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        f.params.output_format = other
        assert validate(f, scenes.palette(8), RR.reflect(4, 1.0)) == abi.SDF_OK


def test_everything_else_is_sdf_validate_materials():
    f, pal, r = frame(), scenes.palette(8), RR.reflect(2, 1.0)
    assert both(f, pal[:7], r) == abi.SDF_E_INVALID_ARG              # not the scene's count
    assert both(frame("C5"), pal[:2], r) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, r, lights=LR.rig(8) + LR.rig(1)) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, r, lights=LR.rig(2), flags=0x2) == abi.SDF_E_INVALID_ARG
    lights = LR.rig(2)
    lights[1].pos[0] = math.nan
    assert both(f, pal, r, lights=lights) == abi.SDF_E_INVALID_ARG
    odd = scenes.palette(8)
    odd[5].shininess = 13.0
    assert both(f, odd, r) == abi.SDF_E_UNSUPPORTED                  # stays UNSUPPORTED
    assert validate(f, pal, r, t=abi.sdf_tiling(0, 0, 1, 0, 1, 1)) == abi.SDF_E_INVALID_ARG
    f.params.samples = 3
    assert both(f, pal, r) == abi.SDF_E_INVALID_ARG
    # the argument checks come first: a bad bounce count on a bad scene
    f = frame()
    f.scene.prims[3].kind = 99
    assert both(f, pal, r) == abi.SDF_E_INVALID_ARG


def test_null_materials_and_lights():
    f = frame()
    r = RR.reflect(1, 1.0)
    marr, n = MR.marr(scenes.palette(8))
    larr = (abi.sdf_light * 1)(f.light)
    head = (C.byref(f.scene), C.byref(f.camera))
    assert lib().sdf_validate_reflect(*head, larr, 1, 0, None, 8, C.byref(r), C.byref(f.params),
                                      None) == abi.SDF_E_INVALID_ARG
    assert lib().sdf_validate_reflect(*head, None, 1, 0, marr, n, C.byref(r), C.byref(f.params),
                                      None) == abi.SDF_E_INVALID_ARG
    assert lib().sdf_render_reflect(*head, None, 1, 0, marr, n, C.byref(r), C.byref(f.params),
                                    None, None, None, None, BOGUS_STREAM) == abi.SDF_E_INVALID_ARG


def test_renderer_signature():
    sig = inspect.signature(R.Renderer.render)
    assert sig.parameters["reflect"].default is None
