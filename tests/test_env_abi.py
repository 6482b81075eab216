"""C-ABI tests of the environment entry points that need no GPU
(include/sdf_abi.h "Environment"): sdf_validate_env and sdf_render_env are
exported with the table's signatures and reject what the header lists with the
documented codes before any device call -- the render entry is handed null
buffers and a stream handle that must never be touched -- the fields of a
feature whose flag is off are ignored, and the ABI version and the other
struct sizes stay as they were."""
import ctypes as C
import inspect
import math

import pytest

import env_ref as ER
import lights_ref as LR
import materials_ref as MR
import reflect_ref as RR
from sdf3d_amd import abi, renderer as R, scenes

BOGUS_STREAM = C.c_void_p(0xDEAD0000BEEF0)     # never dereferenced: every call here is rejected
NULL = object()
SKY, SUN, FOG = abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG
FLAG_SETS = [SKY, SKY | SUN, FOG, SKY | FOG, SKY | SUN | FOG]
BAD = (math.nan, math.inf, -math.inf)


def lib():
    return abi.load_library()


def _args(f, materials, reflect, env, lights, flags):
    lights = [f.light] if lights is None else lights
    larr = (abi.sdf_light * len(lights))(*lights)
    marr, n = MR.marr(materials)
    return (C.byref(f.scene), C.byref(f.camera), larr, len(lights), flags, marr, n,
            None if reflect is NULL else C.byref(reflect), None if env is NULL else C.byref(env),
            C.byref(f.params))


def validate(f, materials, reflect, env, lights=None, flags=0, t=None):
    return lib().sdf_validate_env(*_args(f, materials, reflect, env, lights, flags),
                                  C.byref(t) if t is not None else None)


def render(f, materials, reflect, env, lights=None, flags=0):
    """sdf_render_env with null buffers and the bogus stream."""
    return lib().sdf_render_env(*_args(f, materials, reflect, env, lights, flags), None, None,
                                None, None, BOGUS_STREAM)


def both(f, materials, reflect, env, **kw):
    a, b = validate(f, materials, reflect, env, **kw), render(f, materials, reflect, env, **kw)
    assert a == b, (a, b)
    return a


def frame(cfg="C3"):
    return scenes.config(cfg, *LR.SHAPE)


def test_exports_signatures_and_sizes():
    for name, nargs in (("sdf_validate_env", 11), ("sdf_render_env", 15)):
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert args[7] == C.POINTER(abi.sdf_reflect) and args[8] == C.POINTER(abi.sdf_environment)
        # the rest of the argument order is sdf_render_reflect's
        other = abi.SIGNATURES[name.replace("_env", "_reflect")][1]
        assert args[:8] == other[:8] and args[9:] == other[8:]
        assert hasattr(lib(), name)
    assert C.sizeof(abi.sdf_environment) == 96 == abi.STRUCT_SIZES["sdf_environment"]
    assert [n for n, _ in abi.sdf_environment._fields_] == [
        "flags", "horizon", "zenith", "ground", "sun_dir", "sun_color", "sun_exponent",
        "fog_color", "fog_start", "fog_end", "reserved"]
    assert (abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG) == (1, 2, 4)
    assert lib().sdf_abi_version() == 12 == abi.SDF_ABI_VERSION
    assert C.sizeof(abi.sdf_params) == 80 and C.sizeof(abi.sdf_reflect) == 16


def test_the_default_sky():
    e = scenes.sky()
    assert e.flags == SKY | SUN
    for field in ("horizon", "zenith", "ground", "sun_color", "fog_color"):
        assert all(0.0 <= v <= 1.0 for v in getattr(e, field)), field
    n = math.sqrt(sum(v * v for v in scenes.SKY_SUN_DIR))
    assert list(e.sun_dir) == [C.c_float(v / n).value for v in scenes.SKY_SUN_DIR]
    assert abs(sum(v * v for v in e.sun_dir) - 1.0) < 1e-6 and e.sun_exponent >= 1
    g = scenes.sky(fog=(1.0, 4.0))
    assert g.flags == SKY | SUN | FOG and (g.fog_start, g.fog_end) == (1.0, 4.0)
    assert list(g.fog_color) == list(g.horizon)
    h = scenes.sky(SKY, fog=(0.5, 2.0, (0.25, 0.5, 0.75)))
    assert h.flags == SKY | FOG and list(h.fog_color) == [0.25, 0.5, 0.75]
    t = ER.environment(FOG)
    assert t.flags == FOG and (t.fog_start, t.fog_end) == ER.FOG_RANGE


@pytest.mark.parametrize("cfg", ["REF", "C1", "C2", "C3", "C4", "C5"])
def test_accepts_every_flag_set_bounce_count_and_layer(cfg):
    f = frame(cfg)
    mats = MR.palette_for(f) if cfg != "C5" else [f.material]
    for flags in [0] + FLAG_SETS:
        env = ER.environment(flags)
        for b in range(abi.MAX_BOUNCES + 1):
            for layer in range(-1, b + 1):
                assert validate(f, mats, RR.reflect(b, 0.75, layer), env) == abi.SDF_OK
                if layer >= 0:
                    r = RR.reflect(b, 0.75, layer, abi.REFLECT_WEIGHT)
                    assert validate(f, mats, r, env) == abi.SDF_OK
    assert validate(f, mats, RR.reflect(2, 1.0), NULL) == abi.SDF_OK
    assert validate(f, mats, RR.reflect(3, -2.0), ER.environment(SKY | SUN | FOG), LR.rig(8),
                    abi.LIGHTS_COLOR) == abi.SDF_OK


def test_flag_bits():
    f, pal, r = frame(), scenes.palette(8), RR.reflect(2, 1.0)
    for flags in (0x8, 0x10, 0x9, 0x100, -1, -8, 1 << 30):
        assert both(f, pal, r, ER.environment(flags)) == abi.SDF_E_INVALID_ARG, flags
    # a glow needs a sky to sit on
    assert both(f, pal, r, ER.environment(SUN)) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, r, ER.environment(SUN | FOG)) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, RR.reflect(0, 1.0), ER.environment(SUN)) == abi.SDF_E_INVALID_ARG


def _with(flags, field, index, value):
    e = ER.environment(flags)
    if index is None:
        setattr(e, field, value)
    else:
        getattr(e, field)[index] = value
    return e


SKY_FIELDS = [("horizon", 0), ("zenith", 1), ("ground", 2)]
SUN_FIELDS = [("sun_dir", 1), ("sun_color", 2), ("sun_exponent", None)]
FOG_FIELDS = [("fog_color", 0), ("fog_start", None), ("fog_end", None)]


@pytest.mark.parametrize("bounces", [0, 2])
def test_fields_of_a_feature_that_is_on_are_finite(bounces):
    f, pal, r = frame(), scenes.palette(8), RR.reflect(bounces, 1.0)
    for bad in BAD:
        for field, i in SKY_FIELDS:
            for flags in (SKY, SKY | SUN, SKY | FOG):
                assert both(f, pal, r, _with(flags, field, i, bad)) == abi.SDF_E_INVALID_ARG
        for field, i in SUN_FIELDS:
            for flags in (SKY | SUN, SKY | SUN | FOG):
                assert both(f, pal, r, _with(flags, field, i, bad)) == abi.SDF_E_INVALID_ARG
        for field, i in FOG_FIELDS:
            for flags in (FOG, SKY | SUN | FOG):
                assert both(f, pal, r, _with(flags, field, i, bad)) == abi.SDF_E_INVALID_ARG


def test_sun_exponent_is_at_least_one():
    f, pal, r = frame(), scenes.palette(8), RR.reflect(1, 1.0)
    for x in (0.0, -0.0, 0.5, 0.99999994, -1.0, -64.0):
        assert both(f, pal, r, _with(SKY | SUN, "sun_exponent", None, x)) == abi.SDF_E_INVALID_ARG
    for x in (1.0, 1.5, 12.0, 64.0, 1000.0, 3e38):
        assert validate(f, pal, r, _with(SKY | SUN, "sun_exponent", None, x)) == abi.SDF_OK, x
    # a direction is used as given: any finite one, the null vector included
    for d in ((0.0, 0.0, 0.0), (3.0, -4.0, 12.0), (1e-30, 0.0, -1e30)):
        e = ER.environment(SKY | SUN)
        for c in range(3):
            e.sun_dir[c] = d[c]
        assert validate(f, pal, r, e) == abi.SDF_OK


def test_fog_range_is_not_empty():
    f, pal, r = frame(), scenes.palette(8), RR.reflect(1, 1.0)
    # RN(fog_end - fog_start) must be greater than 0: 1 + 2^-25 - 1 rounds to 0
    for start, end in ((4.0, 1.0), (2.0, 2.0), (0.0, 0.0), (0.0, -0.0), (1e30, 1e30),
                       (-1.0, -3.0)):
        assert both(f, pal, r, ER.environment(FOG, (start, end))) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, r, ER.environment(SKY | FOG, (3.0, 3.0))) == abi.SDF_E_INVALID_ARG
    # ... and neither it nor its reciprocal may overflow: finite ends whose
    # difference is infinite, and a range so narrow that 1 / den is
    for start, end in ((-3e38, 3e38), (0.0, 1e-45), (0.0, 2.9e-39)):
        assert both(f, pal, r, ER.environment(FOG, (start, end))) == abi.SDF_E_INVALID_ARG
    for start, end in ((1.0, 4.0), (-2.0, -1.0), (1.0, 1.0000001), (0.0, 1e30), (0.0, 3e38),
                       (0.0, 3e-39), (-1.7e38, 1.7e38)):
        assert validate(f, pal, r, ER.environment(FOG, (start, end))) == abi.SDF_OK, (start, end)


@pytest.mark.parametrize("bounces", [0, 2])
def test_fields_of_a_feature_that_is_off_are_ignored(bounces):
    f, pal, r = frame(), scenes.palette(8), RR.reflect(bounces, 1.0)
    cases = [(0, SKY_FIELDS + SUN_FIELDS + FOG_FIELDS), (SKY, SUN_FIELDS + FOG_FIELDS),
             (SKY | SUN, FOG_FIELDS), (FOG, SKY_FIELDS + SUN_FIELDS), (SKY | FOG, SUN_FIELDS)]
    for flags, fields in cases:
        for field, i in fields:
            for bad in BAD:
                assert validate(f, pal, r, _with(flags, field, i, bad)) == abi.SDF_OK, (flags, field)
        assert validate(f, pal, r, _with(flags, "reserved", 1, 77)) == abi.SDF_OK
    # an empty fog range and an exponent below 1 likewise
    assert validate(f, pal, r, ER.environment(SKY | SUN, (4.0, 1.0))) == abi.SDF_OK
    assert validate(f, pal, r, _with(SKY | FOG, "sun_exponent", None, 0.0)) == abi.SDF_OK


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_term_streams_carry_no_environment(fmt):
    f = frame()
    f.params.output_format = fmt
    same = [type(f.material).from_buffer_copy(f.material) for _ in range(8)]
    # nothing switched on: sdf_validate_reflect's answer
    for env in (NULL, ER.environment(0)):
        assert validate(f, same, RR.reflect(0, 1.0), env) == abi.SDF_OK
        assert both(f, same, RR.reflect(1, 1.0), env) == abi.SDF_E_UNSUPPORTED
    for flags in FLAG_SETS:
        for r in (RR.reflect(0, 1.0), RR.reflect(0, 1.0, 0), RR.reflect(2, 1.0),
                  RR.reflect(0, 1.0, 0, abi.REFLECT_WEIGHT)):
            assert both(f, same, r, ER.environment(flags)) == abi.SDF_E_UNSUPPORTED
    g = frame("C5")
    g.params.output_format = fmt
    assert both(g, [g.material], RR.reflect(0, 1.0), ER.environment(SKY)) == abi.SDF_E_UNSUPPORTED
    for other in (abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        f.params.output_format = other
        assert validate(f, scenes.palette(8), RR.reflect(0, 1.0),
                        ER.environment(SKY | SUN | FOG)) == abi.SDF_OK


def test_everything_else_is_sdf_validate_reflect():
    f, pal, r, env = frame(), scenes.palette(8), RR.reflect(2, 1.0), ER.environment(SKY | FOG)
    assert both(f, pal, NULL, env) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, NULL, NULL) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, RR.reflect(5, 1.0), env) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, RR.reflect(2, 1.0, 3), env) == abi.SDF_E_INVALID_ARG
    assert both(f, pal, RR.reflect(2, math.nan), env) == abi.SDF_E_INVALID_ARG
    assert both(f, pal[:7], r, env) == abi.SDF_E_INVALID_ARG              # not the scene's count
    assert both(f, pal, r, env, lights=LR.rig(8) + LR.rig(1)) == abi.SDF_E_INVALID_ARG
    bad = scenes.palette(8)
    bad[2].ref[1] = math.nan
    assert both(f, bad, r, env) == abi.SDF_E_INVALID_ARG
    odd = scenes.palette(8)
    odd[5].shininess = 13.0
    assert both(f, odd, r, env) == abi.SDF_E_UNSUPPORTED                  # stays UNSUPPORTED
    assert both(f, odd, r, NULL) == abi.SDF_E_UNSUPPORTED
    assert validate(f, pal, r, env, t=abi.sdf_tiling(0, 0, 1, 0, 1, 1)) == abi.SDF_E_INVALID_ARG
    f.params.samples = 3
    assert both(f, pal, r, env) == abi.SDF_E_INVALID_ARG


def test_renderer_signature():
    sig = inspect.signature(R.Renderer.render)
    assert sig.parameters["env"].default is None
