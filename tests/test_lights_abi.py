"""C-ABI tests of the multi-light entry points that need no GPU
(include/sdf_abi.h "Lights"): sdf_validate_lights and sdf_render_lights are
exported with the table's signatures, reject what the header lists with the
documented codes before any device call, and leave the ABI version and the
struct sizes as they were."""
import ctypes as C
import math

import pytest

import lights_ref as LR
from sdf3d_amd import abi, renderer as R, scenes


def lib():
    return abi.load_library()


def array(lights):
    return (abi.sdf_light * max(len(lights), 1))(*lights)


def validate(f, lights, flags=0, t=None, n=None):
    return lib().sdf_validate_lights(
        C.byref(f.scene), C.byref(f.camera), array(lights) if lights is not None else None,
        len(lights) if n is None else n, flags, C.byref(f.material), C.byref(f.params),
        C.byref(t) if t is not None else None)


def frame(cfg="C3"):
    return scenes.config(cfg, *LR.SHAPE)


def test_exports_and_signatures():
    for name, nargs in (("sdf_validate_lights", 8), ("sdf_render_lights", 12)):
        assert name in abi.SIGNATURES
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert args[2] == C.POINTER(abi.sdf_light) and args[3] is C.c_int32 and args[4] is C.c_int32
        assert hasattr(lib(), name)
    assert abi.MAX_LIGHTS == 8 and abi.LIGHTS_COLOR == 1


def test_version_and_struct_sizes_are_unchanged():
    assert lib().sdf_abi_version() == 12 == abi.SDF_ABI_VERSION
    assert C.sizeof(abi.sdf_params) == 80 and C.sizeof(abi.sdf_light) == 32


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("flags", [0, abi.LIGHTS_COLOR])
def test_accepts_the_rig(n, flags):
    for cfg in scenes.CONFIGS:
        assert validate(scenes.config(cfg), LR.rig(n), flags) == abi.SDF_OK, cfg


def test_null_lights_and_counts():
    f = frame()
    assert validate(f, None, n=1) == abi.SDF_E_INVALID_ARG
    for n in (0, -1, 9, 1 << 30):
        assert validate(f, LR.rig(8), n=n) == abi.SDF_E_INVALID_ARG, n


@pytest.mark.parametrize("flags", [0x2, 0x3, -1, 0x100])
def test_unknown_light_flags(flags):
    assert validate(frame(), LR.rig(2), flags) == abi.SDF_E_INVALID_ARG


@pytest.mark.parametrize("which", [0, 1, 7])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf, 2e15])
def test_bad_light_position(which, bad):
    f = frame()
    lights = LR.rig(8)
    lights[which].pos[1] = bad
    assert validate(f, lights) == abi.SDF_E_INVALID_ARG
    # what sdf_validate says of that light alone
    g = LR.with_light(f, lights[which])
    assert lib().sdf_validate(C.byref(g.scene), C.byref(g.camera), C.byref(g.light),
                              C.byref(g.material), C.byref(g.params), None) == abi.SDF_E_INVALID_ARG


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_colours(bad):
    f = frame()
    lights = LR.rig(3)
    lights[2].color[1] = bad
    assert validate(f, lights, abi.LIGHTS_COLOR) == abi.SDF_E_INVALID_ARG
    assert validate(f, lights, 0) == abi.SDF_OK           # ignored without the flag
    lights[2].color[1] = -3.5                              # any finite factor
    assert validate(f, lights, abi.LIGHTS_COLOR) == abi.SDF_OK


def test_everything_else_is_sdf_validate():
    f = frame()
    f.params.flags |= 0x4                                  # unknown sdf_params.flags bit
    assert validate(f, LR.rig(2)) == abi.SDF_E_INVALID_ARG
    f = frame()
    f.params.samples = 3
    assert validate(f, LR.rig(2)) == abi.SDF_E_INVALID_ARG
    f = frame()
    assert validate(f, LR.rig(2), t=abi.sdf_tiling(0, 0, 1, 0, 1, 1)) == abi.SDF_E_INVALID_ARG


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_term_streams_carry_one_light(fmt):
    f = frame()
    f.params.output_format = fmt
    assert validate(f, LR.rig(2)) == abi.SDF_E_UNSUPPORTED
    assert validate(f, LR.rig(1), abi.LIGHTS_COLOR) == abi.SDF_E_UNSUPPORTED
    assert validate(f, LR.rig(1)) == abi.SDF_OK
    # the other formats take any rig
    for other in (abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        f.params.output_format = other
        assert validate(f, LR.rig(8), abi.LIGHTS_COLOR) == abi.SDF_OK


def test_one_plain_light_validates_where_sdf_validate_does():
    for cfg in scenes.CONFIGS:
        for fmt in (abi.FORMAT_RGBA32F, abi.FORMAT_TILES, abi.FORMAT_SHADE32F):
            for samples in (0, 2):
                f = scenes.config(cfg)
                f.params.output_format = fmt
                f.params.samples = samples
                want = lib().sdf_validate(C.byref(f.scene), C.byref(f.camera), C.byref(f.light),
                                          C.byref(f.material), C.byref(f.params), None)
                assert validate(f, [f.light]) == want, (cfg, fmt, samples)


def test_render_rejects_before_any_device_call():
    """sdf_render_lights validates first: with null buffers and no device the
    rejections come back as from sdf_validate_lights."""
    f = frame()
    call = lib().sdf_render_lights

    def render(lights, n, flags):
        return call(C.byref(f.scene), C.byref(f.camera), array(lights) if lights else None, n,
                    flags, C.byref(f.material), C.byref(f.params), None, None, None, None, None)
    assert render(None, 1, 0) == abi.SDF_E_INVALID_ARG
    assert render(LR.rig(8), 9, 0) == abi.SDF_E_INVALID_ARG
    assert render(LR.rig(2), 2, 0x2) == abi.SDF_E_INVALID_ARG
    f.params.output_format = abi.FORMAT_SHADE32F
    assert render(LR.rig(2), 2, 0) == abi.SDF_E_UNSUPPORTED


def test_renderer_signature():
    import inspect
    sig = inspect.signature(R.Renderer.render)
    assert sig.parameters["lights"].default is None
    assert sig.parameters["light_flags"].default == 0
