"""The rays entry points at the C-ABI boundary, without a device
(include/sdf_abi.h "Rays"): the symbols exist, sdf_rays has its layout, every
SDF_E_INVALID_ARG and SDF_E_UNSUPPORTED case is decided before any device call
-- through sdf_validate_rays and through sdf_render_rays, which is handed a
stream handle that must never be touched -- n = 0 is SDF_OK on a machine with
no GPU, and the two NumPy ray generators of sdf3d_amd.camera give the rays they
document."""
import ctypes as C
import math

import numpy as np
import pytest

import env_ref as ER
import lights_ref as LR
import materials_ref as MR
import reflect_ref as RR
from sdf3d_amd import abi, camera, scenes

OK, INVALID, UNSUPPORTED = abi.SDF_OK, abi.SDF_E_INVALID_ARG, abi.SDF_E_UNSUPPORTED
PTR = 0x1000   # a non-null "device pointer": never dereferenced before a device call
BOGUS_STREAM = C.c_void_p(0xDEAD0000BEEF0)     # never dereferenced: every call here is rejected
NULL = object()
SKY, SUN, FOG = abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame(name="C4"):
    return scenes.config(name, 64, 36)


def mats_of(f):
    return MR.palette_for(f) if f.scene.kind == abi.SCENE_PRIMITIVES else [f.material]


def rays_of(origins=PTR, dirs=PTR, n=1, flags=0):
    return abi.sdf_rays(origins, dirs, n, flags, 0)


def call(lib, f, rays=None, materials=None, reflect=NULL, env=NULL, lights=None, light_flags=0,
         scene=True, params=True, rgba=PTR, render=True):
    """sdf_validate_rays (render False) or sdf_render_rays with the bogus stream."""
    rays = rays_of() if rays is None else rays
    lights = [f.light] if lights is None else lights
    larr = (abi.sdf_light * max(len(lights), 1))(*lights)
    marr, nm = MR.marr(mats_of(f) if materials is None else materials)
    head = (C.byref(f.scene) if scene else None, larr if lights else None, len(lights),
            light_flags, marr, nm, None if reflect is NULL else C.byref(reflect),
            None if env is NULL else C.byref(env), C.byref(f.params) if params else None,
            None if rays is NULL else C.byref(rays))
    if not render:
        return lib.sdf_validate_rays(*head)
    return lib.sdf_render_rays(*head, rgba, None, BOGUS_STREAM)


def both(lib, f, **kw):
    a, b = call(lib, f, render=False, **kw), call(lib, f, render=True, **kw)
    assert a == b, (a, b)
    return a


def test_symbols_and_layout(lib):
    for name, nargs in (("sdf_validate_rays", 10), ("sdf_render_rays", 13), ("sdf_camera_rays", 5)):
        assert hasattr(lib, name), name
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    assert C.sizeof(abi.sdf_rays) == 32 == abi.STRUCT_SIZES["sdf_rays"]
    assert [n for n, _ in abi.sdf_rays._fields_] == ["origins", "dirs", "n", "flags", "reserved"]
    assert abi.sdf_rays.n.offset == 16 and abi.sdf_rays.flags.offset == 24
    assert abi.RAYS_UNIT == 1
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


@pytest.mark.parametrize("cfg", ["REF", "C1", "C2", "C3", "C4", "C5"])
def test_accepts_every_config_with_and_without_reflect_and_env(lib, cfg):
    f = frame(cfg)
    for unit in (0, abi.RAYS_UNIT):
        r = rays_of(flags=unit)
        assert call(lib, f, r, render=False) == OK                     # reflect NULL, env NULL
        assert call(lib, f, r, reflect=RR.reflect(2, 0.75), render=False) == OK
        assert call(lib, f, r, env=ER.environment(SKY | SUN | FOG), render=False) == OK
        assert call(lib, f, r, reflect=RR.reflect(3, 1.0, 1, abi.REFLECT_WEIGHT),
                    env=ER.environment(FOG), lights=LR.rig(3), light_flags=abi.LIGHTS_COLOR,
                    render=False) == OK
        assert call(lib, f, r, env=ER.environment(0), render=False) == OK
    for fmt in (abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        g = f.copy()
        g.params.output_format = fmt
        assert call(lib, g, render=False) == OK


def test_invalid_arguments_before_any_device_call(lib):
    f = frame()
    assert both(lib, f, rays=NULL) == INVALID
    assert both(lib, f, scene=False) == INVALID
    assert both(lib, f, params=False) == INVALID
    for flags in (0x2, 0x3, 0x100, -1, 1 << 30):
        assert both(lib, f, rays=rays_of(flags=flags)) == INVALID, flags
    assert both(lib, f, rays=rays_of(n=-1)) == INVALID
    assert both(lib, f, rays=rays_of(n=(1 << 30) + 1)) == INVALID
    assert both(lib, f, rays=rays_of(origins=None)) == INVALID
    assert both(lib, f, rays=rays_of(dirs=None)) == INVALID
    assert call(lib, f, rgba=None) == INVALID                         # NULL rgba with n > 0
    assert call(lib, f, rays=rays_of(n=1 << 30), render=False) == OK     # n at the limit is legal
    assert both(lib, f, lights=[]) == INVALID
    # anything the validators below reject, n = 0 included
    g = f.copy()
    g.params.max_steps = -1
    assert both(lib, g) == INVALID and both(lib, g, rays=rays_of(n=0)) == INVALID
    g = f.copy()
    g.scene.prims[2].p[0] = float("nan")
    assert both(lib, g) == INVALID
    assert both(lib, f, materials=mats_of(f)[:-1]) == INVALID         # one material per primitive
    assert both(lib, f, lights=LR.rig(8) + [f.light]) == INVALID      # too many lights
    assert both(lib, f, light_flags=0x2) == INVALID
    g = f.copy()
    g.params.samples = 3
    assert both(lib, g) == INVALID


def test_an_invalid_reflect_or_env_gives_sdf_validate_envs_code(lib):
    f = frame()
    mats = mats_of(f)
    larr = (abi.sdf_light * 1)(f.light)
    marr, nm = MR.marr(mats)

    def env_code(reflect, env):
        return lib.sdf_validate_env(C.byref(f.scene), C.byref(f.camera), larr, 1, 0, marr, nm,
                                    C.byref(reflect), C.byref(env), C.byref(f.params), None)
    cases = [(RR.reflect(-1, 1.0), ER.environment(0)), (RR.reflect(5, 1.0), ER.environment(0)),
             (RR.reflect(2, 1.0, 3), ER.environment(SKY)), (RR.reflect(2, 1.0, -2), ER.environment(0)),
             (RR.reflect(2, 1.0, -1, abi.REFLECT_WEIGHT), ER.environment(0)),
             (RR.reflect(2, 1.0, 0, 0x2), ER.environment(0)),
             (RR.reflect(2, math.nan), ER.environment(SKY)),
             (RR.reflect(1, 1.0), ER.environment(0x8)), (RR.reflect(1, 1.0), ER.environment(SUN)),
             (RR.reflect(1, 1.0), ER.environment(FOG, fog=(2.0, 2.0))),
             (RR.reflect(1, 1.0), ER.environment(FOG, fog=(0.0, math.inf)))]
    e = ER.environment(SKY)
    e.zenith[1] = math.nan
    cases.append((RR.reflect(0, 1.0), e))
    e = ER.environment(SKY | SUN)
    e.sun_exponent = 0.5
    cases.append((RR.reflect(0, 1.0), e))
    for reflect, env in cases:
        want = env_code(reflect, env)
        assert want == INVALID
        assert both(lib, f, reflect=reflect, env=env) == want
    # fields of a feature whose flag is off are ignored, as there
    e = ER.environment(FOG)
    e.zenith[0] = e.sun_exponent = math.nan
    assert env_code(RR.reflect(1, 1.0), e) == OK
    assert call(lib, f, reflect=RR.reflect(1, 1.0), env=e, render=False) == OK


def test_unsupported(lib):
    f = frame()
    for s in (2, 4):
        g = f.copy()
        g.params.samples = s
        assert both(lib, g) == UNSUPPORTED
        assert both(lib, g, reflect=RR.reflect(2, 1.0), env=ER.environment(SKY)) == UNSUPPORTED
    for fmt in (abi.FORMAT_TILES, abi.FORMAT_SHADE32F):
        g = f.copy()
        g.params.output_format = fmt
        one = [f.material] * f.scene.count
        assert both(lib, g, materials=one) == UNSUPPORTED      # even where sdf_render takes it
        assert both(lib, g) == UNSUPPORTED
        assert both(lib, g, reflect=RR.reflect(2, 1.0), env=ER.environment(SKY)) == UNSUPPORTED
    # sdf_validate_env's own SDF_E_UNSUPPORTED cases stay: the exponent is frame-wide
    mats = mats_of(f)
    mats[1].shininess = 20.0
    assert both(lib, f, materials=mats) == UNSUPPORTED


def test_width_height_play_no_part(lib):
    f = frame()
    f.params.width, f.params.height = -5, 1 << 20
    f.camera.eye[0] = float("nan")              # no camera is looked at either
    assert call(lib, f, render=False) == OK
    assert call(lib, f, rays=rays_of(n=0)) == OK


def test_nothing_to_do_needs_no_device(lib):
    """n = 0 launches nothing and touches no buffer: SDF_OK without a GPU, with
    garbage and with null pointers."""
    for name in ("REF", "C4", "C5"):
        f = frame(name)
        for r in (rays_of(n=0), rays_of(None, None, 0), rays_of(0xDEAD0000, 0xBEEF0000, 0)):
            assert call(lib, f, rays=r) == OK
            assert call(lib, f, rays=r, rgba=None) == OK
            assert call(lib, f, rays=r, rgba=0xDEAD0000, reflect=RR.reflect(2, 1.0),
                        env=ER.environment(SKY | FOG)) == OK
            assert call(lib, f, rays=r, render=False) == OK


def test_camera_rays_rejections(lib):
    f = frame()

    def cam(fr=f, camera=True, params=True, o=PTR, d=PTR):
        return lib.sdf_camera_rays(C.byref(fr.camera) if camera else None,
                                   C.byref(fr.params) if params else None, o, d, BOGUS_STREAM)
    assert cam(camera=False) == INVALID
    assert cam(params=False) == INVALID
    assert cam(o=None, d=None) == INVALID
    for field, bad in (("width", 0), ("height", -3), ("precision", 2)):
        g = f.copy()
        setattr(g.params, field, bad)
        assert cam(g) == INVALID, field
    g = f.copy()
    g.camera.eye[0] = float("nan")
    assert cam(g) == INVALID
    g = f.copy()
    g.camera.fov_deg = float("inf")
    assert cam(g) == INVALID
    for s in (2, 4):
        g = f.copy()
        g.params.samples = s
        assert cam(g) == UNSUPPORTED


def test_renderer_checks_its_tensors():
    """Renderer.render_rays refuses anything but contiguous float32 (n, 3)
    tensors, a wrong output or steps tensor and a stream format, before any
    call (a stand-in renderer: no GPU)."""
    import torch
    from sdf3d_amd.renderer import Renderer
    rd = Renderer.__new__(Renderer)
    rd.torch, rd.device, rd.lib = torch, torch.device("cpu"), None
    f = frame()
    good = torch.zeros((4, 3), dtype=torch.float32)
    for bad in (good.double(), torch.zeros((4, 4)), torch.zeros((3, 4)).t(), torch.zeros(12),
                good.numpy()):
        with pytest.raises(ValueError):
            rd.render_rays(f, bad, good)
        with pytest.raises(ValueError):
            rd.render_rays(f, good, bad)
    with pytest.raises(ValueError):
        rd.render_rays(f, good, torch.zeros((5, 3)))
    with pytest.raises(ValueError):
        rd.render_rays(f, good, good, out=torch.zeros((4, 3)))
    with pytest.raises(ValueError):
        rd.render_rays(f, good, good, steps=torch.zeros((4, 2)))
    g = f.copy()
    g.params.output_format = abi.FORMAT_TILES
    with pytest.raises(ValueError):
        rd.render_rays(g, good, good)


# ---- the NumPy ray generators (sdf3d_amd/camera.py) ---------------------------------

def unit_error(d):
    return np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max()


def test_ortho_rays():
    w, h, hh = 37, 23, 1.5
    f = scenes.config("C3", w, h)                  # the default camera: identity view
    o, d = camera.ortho_rays(f, hh)
    assert o.shape == d.shape == (h, w, 3) and o.dtype == d.dtype == np.float32
    assert o.flags.c_contiguous and d.flags.c_contiguous
    assert unit_error(d) <= 1e-6
    assert (d == np.array([0.0, 0.0, -1.0], dtype=np.float32)).all()   # along the view direction
    eye = np.array(list(f.camera.eye))
    assert np.allclose(o[h // 2, w // 2], eye, atol=1e-6)              # odd sizes: the centre pixel
    ax = hh * w / h
    assert np.allclose(o[0, 0], eye + [-(1 - 1 / w) * ax, -(1 - 1 / h) * hh, 0], atol=1e-6)
    assert np.allclose(o[-1, -1], eye + [(1 - 1 / w) * ax, (1 - 1 / h) * hh, 0], atol=1e-6)
    # an orbited camera with an aspect of its own: the rays turn with it
    g = scenes.config("C3", w, h, pose=2)          # yaw -30, pitch 10
    g.camera.aspect = 2.0
    o2, d2 = camera.ortho_rays(g, hh)
    inv = np.linalg.inv(np.array(list(g.camera.view), dtype=np.float64).reshape(4, 4).T)
    assert unit_error(d2) <= 1e-6
    assert np.allclose(d2, -inv[:3, 2], atol=1e-6)
    assert np.allclose(o2[h // 2, w // 2], inv[:3, :3] @ eye + inv[:3, 3], atol=1e-6)
    span = o2[0, -1].astype(np.float64) - o2[0, 0]
    assert np.allclose(span, inv[:3, 0] * 2 * (1 - 1 / w) * hh * 2.0, atol=1e-5)
    assert np.abs((o2 - o2[h // 2, w // 2]) @ d2[0, 0]).max() <= 1e-5    # one plane through the eye


def test_equirect_rays():
    w, h = 37, 23
    eye = (0.25, 0.5, -1.0)
    o, d = camera.equirect_rays(eye, w, h)
    assert o.shape == d.shape == (h, w, 3) and o.dtype == d.dtype == np.float32
    assert o.flags.c_contiguous and d.flags.c_contiguous
    assert (o == np.array(eye, dtype=np.float32)).all()
    assert unit_error(d) <= 1e-6
    assert np.allclose(d[h // 2, w // 2], [0, 0, -1], atol=1e-6)      # the centre looks along -z
    lat = (1 - 1 / h) * math.pi / 2                                    # the outermost pixel centres
    lon = (1 - 1 / w) * math.pi
    want = [math.cos(lat) * math.sin(lon), math.sin(lat), -math.cos(lat) * math.cos(lon)]
    assert np.allclose(d[-1, -1], want, atol=1e-6)                     # top right: up, behind
    assert np.allclose(d[0, 0], [-want[0], -want[1], want[2]], atol=1e-6)
    assert math.degrees(lat) > 86 and d[-1, :, 1].min() > 0.997        # the top row: near the zenith
    assert np.allclose(d[h // 2, 0], [-math.sin(lon), 0, -math.cos(lon)], atol=1e-6)
    # longitude across, latitude up
    assert (np.diff(d[:, w // 2, 1]) > 0).all()
    assert (np.diff(np.arctan2(d[h // 2, :, 0], -d[h // 2, :, 2])) > 0).all()
