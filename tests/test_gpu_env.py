"""GPU tests of the environment (sdf_render_env; include/sdf_abi.h
"Environment"): in exact precision the composite and its summed step counts
bit for bit and on every pixel against the CPU reference (tests/env_ref.py),
every single layer and weight plane with it; in both precisions the composite
against the composition of the kernel's own layers and weights; nothing
switched on is sdf_render_reflect; within a measured bound against the
reference in fast precision -- on every dispatch path, for every output format,
tiling, a schedule and supersampling.

Shape 37 x 23 (partial 8 x 8 tiles in x and y, a last block of 7 rows); the
supersampled cases use cases.SHAPES.  Every render writes into
buffers followed by sentinel rows, which must survive, and every case is
rendered with and without a steps buffer, which must not change the colours.
The environment is env_ref.environment: scenes.sky() with fog from 1 to 4 in
the horizon's colour."""
import ctypes as C
import os

import numpy as np
import pytest

import env_ref as ER
import gpu_support as G
import materials_ref as MR
import reflect_ref as RR
import ssaa_ref
from cases import LIGHTS, env_scene, fast_case, mats_of, the_frame, walk_of
from fast_paths import ALL, WEIGHT
from fast_paths import ENV_BOUND as FAST_BOUND
from gpu_support import (FILL, SHAPES, bits, fenced, hi_frame, ndiff, read_ppm, rgba_of, same,
                         sdf_main, untouched)
from sdf3d_amd import abi, renderer as R, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
PRECS = [EXACT, FAST]
SKY, SUN, FOG = abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG
FLAG_SETS = [SKY, SKY | SUN, FOG, ALL]
FRAMES = MR.FRAMES + [("C5", 0)]
RIGS = [(1, 0), (3, abi.LIGHTS_COLOR)]

def shading(reflect, env, materials=None, lights=None, flags=0):
    return dict(reflect=reflect, env=env, materials=materials, lights=lights, light_flags=flags)


def render(rd, frame, reflect, env, materials=None, lights=None, flags=0, t=None, steps=True,
           schedule=None):
    """gpu_support.render with `env`: sdf_render_env; env None: sdf_render_reflect."""
    return G.render(rd, frame, t, steps, schedule, **shading(reflect, env, materials, lights, flags))


def both(rd, frame, reflect, env, materials=None, lights=None, flags=0, t=None):
    return G.both(rd, frame, t, **shading(reflect, env, materials, lights, flags))


# ---- the reference: one walk per case, the environments applied to it -------------

_REF = {}


def reference(name, pose, bounces, n, flags, eflags, fog=ER.FOG_RANGE):
    key = (name, pose, bounces, n, flags, eflags, fog)
    if key not in _REF:
        f = the_frame(name, pose)
        e = ER.apply(f, walk_of(name, pose, bounces, n, flags), ER.environment(eflags, fog))
        rgba = RR.composite(e["C"], e["W"], e["alive"])
        assert np.isfinite(rgba).all(), key
        steps = e["steps"].sum(axis=2).astype(np.int32)
        for a in (rgba, steps, *e.values()):
            a.setflags(write=False)
        _REF[key] = (rgba, steps, e)
    return _REF[key]


def check_reference(rd, name, pose, bounces, n, flags, eflags, dispatch=None, layers=False,
                    fog=ER.FOG_RANGE):
    """The exact composite and its summed steps are the reference's on every
    pixel; `layers`: so is every layer and every weight plane, with the layer's
    own steps."""
    f = the_frame(name, pose, EXACT, dispatch)
    want, want_st, e = reference(name, pose, bounces, n, flags, eflags, fog)
    env = ER.environment(eflags, fog)
    mats, lights = mats_of(f), LIGHTS[:n]
    out, st = both(rd, f, RR.reflect(bounces, 1.0), env, mats, lights, flags)
    print(f"differing words {ndiff(out, want)} of {out.size}; sky layers {int(e['sky'].sum())}, "
          f"fogged layers {int(((e['f'] < 1) & e['alive']).sum())}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, want_st)
    if not layers:
        return
    for j in range(bounces + 1):
        cj, sj = both(rd, f, RR.reflect(bounces, 1.0, j), env, mats, lights, flags)
        assert same(cj, rgba_of(e["C"][:, :, j])), j
        assert np.array_equal(sj, e["steps"][:, :, j]), j
        wj, wsj = both(rd, f, RR.reflect(bounces, 1.0, j, WEIGHT), env, mats, lights, flags)
        assert same(wj, rgba_of(e["W"][:, :, j])), j
        assert np.array_equal(wsj, e["steps"][:, :, j]), j


# ---- 1. exact precision against the reference -----------------------------------

@pytest.mark.parametrize("n,flags", RIGS)
@pytest.mark.parametrize("bounces", [0, 2])
@pytest.mark.parametrize("eflags", FLAG_SETS)
@pytest.mark.parametrize("name,pose", FRAMES)
def test_exact_equals_reference(renderer, name, pose, eflags, bounces, n, flags):
    check_reference(renderer, name, pose, bounces, n, flags, eflags)


@pytest.mark.parametrize("eflags", [SKY | SUN, ALL])
@pytest.mark.parametrize("name,pose", [("REF", 0), ("C2", 1), ("C4", 0), ("SIX", 2), ("C5", 0)])
def test_exact_layers_and_weights_equal_reference(renderer, name, pose, eflags):
    """One frame per scene class: the two small built-in scenes, the built-in
    CSG8 scene, the generic kernel and the Mandelbulb (a run-time compiled
    scene: test_paths_exact_equals_reference, EJ)."""
    check_reference(renderer, name, pose, 2, 3, abi.LIGHTS_COLOR, eflags, layers=True)


# ---- 2. both precisions, from the kernel's own pieces ----------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,pose,n,flags", [("C4", 0, 2, abi.LIGHTS_COLOR), ("SIX", 2, 1, 0),
                                               ("C5", 0, 2, abi.LIGHTS_COLOR)])
def test_composite_is_the_fold_of_own_layers(renderer, name, pose, n, flags, prec):
    f = the_frame(name, pose, prec)
    mats, lights, env = mats_of(f), LIGHTS[:n], ER.environment(ALL)
    Cj, Wj, Sj, alive = G.own_layers(lambda r: both(renderer, f, r, env, mats, lights, flags), 3, 0.75)
    assert alive[:, :, 0].all() and (bits(Wj[:, :, 0]) == bits(np.ones(3, f32))).all()
    assert alive[:, :, 1].mean() > 0.02
    out, st = both(renderer, f, RR.reflect(3, 0.75), env, mats, lights, flags)
    want = RR.composite(Cj, Wj, alive, prec)
    print(f"differing words {ndiff(out, want)} of {out.size}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, Sj.sum(axis=2))


# ---- 3. forwarding and degenerate frames --------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("fmt", [abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8,
                                 abi.FORMAT_RGB32F])
def test_nothing_switched_on_is_sdf_render_reflect(renderer, fmt, prec):
    f = the_frame("C4", 0, prec)
    f.params.output_format = fmt
    mats, lights = mats_of(f), LIGHTS[:3]
    none = ER.environment(0)
    for r in (RR.reflect(2, 0.75), RR.reflect(2, 0.75, 1), RR.reflect(2, 0.75, 2, WEIGHT),
              RR.reflect(0, 1.0)):
        want, want_st = both(renderer, f, r, None, mats, lights, abi.LIGHTS_COLOR)
        out, st = both(renderer, f, r, none, mats, lights, abi.LIGHTS_COLOR)
        assert same(out, want) and np.array_equal(st, want_st)
    # env = NULL through the entry point itself
    import torch
    p = f.params
    shape = (p.height, p.width, R.channels(fmt))
    r = RR.reflect(2, 0.75)
    larr = (abi.sdf_light * 3)(*lights)
    marr, nm = MR.marr(mats)
    want, want_st = both(renderer, f, r, None, mats, lights, abi.LIGHTS_COLOR)
    for steps in (False, True):
        buf = fenced(torch, renderer.device, shape, R.torch_dtype(fmt))
        sbuf = fenced(torch, renderer.device, (p.height, p.width, 2), torch.int32)
        rc = renderer.lib.sdf_render_env(
            C.byref(f.scene), C.byref(f.camera), larr, 3, abi.LIGHTS_COLOR, marr, nm, C.byref(r),
            None, C.byref(p), None, C.c_void_p(buf.data_ptr()),
            C.c_void_p(sbuf.data_ptr()) if steps else None, None, None)
        assert rc == abi.SDF_OK
        torch.cuda.synchronize()
        assert same(buf.cpu().numpy(), want) and untouched(torch, buf)
        assert untouched(torch, sbuf)
        if steps:
            assert np.array_equal(sbuf.cpu().numpy(), want_st)
        else:
            assert (bits(sbuf.cpu().numpy()) == FILL).all(), \
                "a null steps pointer: nothing is written"


@pytest.mark.parametrize("prec", PRECS)
def test_term_streams_with_nothing_switched_on(renderer, prec):
    import torch
    f = the_frame("C4", 0, prec)
    f.params.output_format = abi.FORMAT_TILES
    mats = [type(f.material).from_buffer_copy(f.material) for _ in range(f.scene.count)]
    kw = dict(lights=[LIGHTS[1]], materials=mats, reflect=(0, 1.0))
    a, b, n = G.tiles_streams(renderer, f, kw, dict(kw, env=ER.environment(0)))
    for fl in FLAG_SETS:
        with pytest.raises(abi.SdfError) as e:
            renderer.render(f, out=b, env=ER.environment(fl), **kw)
        assert e.value.code == abi.SDF_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(a[:n], b[:n]), "a refused render wrote to its buffer"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("eflags", [SKY, SKY | SUN, ALL])
def test_a_frame_of_sky(renderer, eflags, prec):
    """The camera pitched up: every pixel misses at layer 0, is sky(D) exactly
    (in exact precision the reference's bits) and counts no shadow step."""
    f = ER.sky_frame(prec)
    mats, lights, env = mats_of(f), LIGHTS[:3], ER.environment(eflags)
    out, st = both(renderer, f, RR.reflect(2, 1.0), env, mats, lights, abi.LIGHTS_COLOR)
    assert (st[..., 1] == 0).all() and (st[..., 0] > 0).all()
    assert (out[..., 3] == 1).all() and np.isfinite(out).all()
    one, st1 = both(renderer, f, RR.reflect(2, 1.0, 1), env, mats, lights, abi.LIGHTS_COLOR)
    assert (bits(one[..., :3]) == 0).all() and (st1 == 0).all()
    none, st0 = both(renderer, f, None, env, mats, lights, abi.LIGHTS_COLOR)   # bounces 0
    assert same(none, out) and np.array_equal(st0, st)
    if prec == EXACT:
        g = ER.sky_frame()
        w = RR.walk(g, mats, 0, 1.0, lights)
        assert (w["d"][:, :, 0] > g.params.max_dist).all()
        assert same(out, rgba_of(ER.sky(w["D"][:, :, 0], env)))
        assert np.array_equal(st[..., 0], w["sp"][:, :, 0])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("eflags", [FOG, ALL])
def test_a_frame_of_fog(renderer, eflags, prec):
    """fog_end below the nearest surface: every pixel that is not sky is the
    fog colour's bits, and every path ends at layer 0."""
    f = the_frame("C4", 0, prec)
    w = walk_of("C4", 0, 0, 1, 0)
    assert float(w["d"].min()) > 0.5
    env = ER.environment(eflags, (0.125, 0.25))
    mats, lights = mats_of(f), LIGHTS[:2]
    out, st = both(renderer, f, RR.reflect(2, 1.0), env, mats, lights, abi.LIGHTS_COLOR)
    miss = w["d"][:, :, 0] > f.params.max_dist
    fogged = ~miss if eflags & SKY else np.ones_like(miss)
    assert (bits(out[..., :3][fogged]) == bits(ER.v3(env.fog_color))).all()
    assert (out[..., 3] == 1).all()
    one, st1 = both(renderer, f, RR.reflect(2, 1.0, 1), env, mats, lights, abi.LIGHTS_COLOR)
    assert (bits(one[..., :3]) == 0).all() and (st1 == 0).all()
    wt, _ = both(renderer, f, RR.reflect(2, 1.0, 1, WEIGHT), env, mats, lights, abi.LIGHTS_COLOR)
    assert (bits(wt[..., :3]) == 0).all()
    zero, st0 = both(renderer, f, RR.reflect(0, 1.0), env, mats, lights, abi.LIGHTS_COLOR)
    assert same(zero, out) and np.array_equal(st0, st)


# ---- 4. dispatch paths -------------------------------------------------------------

PATHS = [("SIX", 2, abi.DISPATCH_UNCULLED), ("C4", 0, abi.DISPATCH_GENERIC),
         ("C4", 0, abi.DISPATCH_AUTO), ("C3", 2, abi.DISPATCH_UNCULLED),
         ("REF", 0, abi.DISPATCH_AUTO), ("C2", 1, abi.DISPATCH_AUTO),
         ("EJ", 2, abi.DISPATCH_AUTO), ("EJ", 2, abi.DISPATCH_GENERIC), ("C5", 0, None)]


@pytest.mark.parametrize("name,pose,dispatch", PATHS)
def test_paths_exact_equals_reference(renderer, name, pose, dispatch):
    e = reference(name, pose, 2, 3, abi.LIGHTS_COLOR, ALL)[2]
    assert e["sky"].sum() > 50 and ((e["f"] < 1) & (e["f"] > 0) & e["alive"]).sum() > 50
    check_reference(renderer, name, pose, 2, 3, abi.LIGHTS_COLOR, ALL, dispatch,
                    layers=name == "EJ")


@pytest.mark.parametrize("prec", PRECS)
def test_runtime_specialised_scene_compiles_one_kernel(renderer, prec):
    """A scene without a built-in variant: one run-time compiled env kernel
    serves every set of flags, bounce count, layer and strength (one more with
    step recording, one more with supersampling), beside the reflect kernel of
    the same scene.  In exact precision its frame is the generic kernel's.
    (The renders that are counted run in one mode each: step recording is
    another instantiation, so a second mode would compile a second kernel.
    Both modes are then compared on the 2-bounce frame and on every layer.)"""
    f = env_scene(prec, counted=True)
    mats, lights = mats_of(f), LIGHTS[:2]
    jit = os.environ.get("SDF3D_JIT") != "0"
    count = renderer.lib.sdf_jit_count
    generic = f.copy()
    generic.params.dispatch = abi.DISPATCH_GENERIC
    env = ER.environment(ALL)
    want, want_st = both(renderer, generic, RR.reflect(2, 0.75), env, mats, lights)
    before = count()
    for b, s, layer, fl, ef in ((2, 0.75, -1, 0, ALL), (0, 0.75, -1, 0, SKY), (4, 0.5, -1, 0, FOG),
                                (3, 1.0, 2, 0, SKY | SUN), (3, 1.0, 1, WEIGHT, ALL)):
        render(renderer, f, RR.reflect(b, s, layer, fl), ER.environment(ef), mats, lights,
               steps=False)
        assert count() - before == (1 if jit else 0)
    out, _ = render(renderer, f, RR.reflect(2, 0.75), env, mats, lights, steps=False)
    assert prec == FAST or same(out, want)
    out2, st = render(renderer, f, RR.reflect(2, 0.75), env, mats, lights, steps=True)
    assert same(out2, out) and np.array_equal(st, want_st)
    assert count() - before == (2 if jit else 0)
    Cj, Wj, Sj, alive = G.own_layers(lambda r: both(renderer, f, r, env, mats, lights, 0), 2, 0.75)
    assert same(out, RR.composite(Cj, Wj, alive, prec)) and np.array_equal(st, Sj.sum(axis=2))
    assert count() - before == (2 if jit else 0)
    # nothing switched on is the reflect kernel of this scene: another kernel
    render(renderer, f, RR.reflect(2, 0.75), ER.environment(0), mats, lights, steps=False)
    assert count() - before == (3 if jit else 0)
    g = f.copy()
    g.params.width, g.params.height, g.params.samples = SHAPES[2][0], SHAPES[2][1], 2
    render(renderer, g, RR.reflect(2, 0.75), env, mats, lights, steps=False)
    render(renderer, g, RR.reflect(1, 0.25), ER.environment(SKY), mats, lights, steps=False)
    assert count() - before == (4 if jit else 0)


# ---- 5. formats, tilings, schedule, supersampling -----------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_formats_convert_the_composite(renderer, prec):
    f = the_frame("C4", 0, prec)
    mats, lights, env = mats_of(f), LIGHTS[:2], ER.environment(ALL)
    r = RR.reflect(2, 1.0)
    full, _ = render(renderer, f, r, env, mats, lights, abi.LIGHTS_COLOR, steps=False)
    plain, _ = render(renderer, f, r, None, mats, lights, abi.LIGHTS_COLOR, steps=False)
    assert np.abs(full - plain).max() > 0.1
    if prec == EXACT:
        assert same(full, reference("C4", 0, 2, 2, abi.LIGHTS_COLOR, ALL)[0])
    G.check_formats(renderer, f, full, **shading(r, env, mats, lights, abi.LIGHTS_COLOR))


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_term_streams_are_refused(renderer, fmt):
    import torch
    f = the_frame("C4", 0)
    f.params.output_format = fmt
    mats = [type(f.material).from_buffer_copy(f.material) for _ in range(f.scene.count)]
    if fmt == abi.FORMAT_TILES:
        out = torch.zeros(R.tiles_bytes(f.params.width, f.params.height), dtype=torch.uint8,
                          device=renderer.device)
    else:
        out = torch.zeros((f.params.height, f.params.width, 4), dtype=torch.float32,
                          device=renderer.device)
    for fl in FLAG_SETS:
        for r in (RR.reflect(0, 1.0), RR.reflect(2, 1.0), RR.reflect(2, 1.0, 0)):
            with pytest.raises(abi.SdfError) as e:
                renderer.render(f, out=out, materials=mats, reflect=r, env=ER.environment(fl))
            assert e.value.code == abi.SDF_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any(), "a refused render wrote to its buffer"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("world,shares", [(3, (1, 1)), (2, (1, 2))])
def test_tilings(renderer, world, shares, prec):
    f = the_frame("C3", 2, prec)
    mats, lights, flags, env = mats_of(f), LIGHTS[:2], abi.LIGHTS_COLOR, ER.environment(ALL)
    r = RR.reflect(2, 1.0)
    whole, _ = G.check_tilings(renderer, f, world, shares, **shading(r, env, mats, lights, flags))
    if prec == EXACT:
        assert same(whole, reference("C3", 2, 2, 2, flags, ALL)[0])


@pytest.mark.parametrize("prec", PRECS)
def test_scheduled(renderer, prec):
    f = the_frame("C3", 2, prec)
    mats, lights, env = mats_of(f), LIGHTS[:2], ER.environment(ALL)
    r = RR.reflect(2, 1.0)
    G.check_scheduled(renderer, f, **shading(r, env, mats, lights))


_HI = {}


def hi_reference(name, s):
    """The exact reference of the S W x S H frame of a supersampled case."""
    if (name, s) not in _HI:
        f = MR.frame_of(name, 2, EXACT, wh=SHAPES[s])
        f.params.samples = s
        f = hi_frame(f)
        if name == "SIX":
            f.params.dispatch = abi.DISPATCH_GENERIC
        rgba, steps, _ = ER.render(f, mats_of(f), 2, 1.0, ER.environment(ALL), LIGHTS[:2],
                                   abi.LIGHTS_COLOR)
        _HI[(name, s)] = (rgba, steps)
    return _HI[(name, s)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["C3", "SIX"])
def test_supersampled(renderer, name, s, prec):
    f = MR.frame_of(name, 2, prec, wh=SHAPES[s])
    if name == "SIX":
        f.params.dispatch = abi.DISPATCH_GENERIC
    f.params.samples = s
    mats, lights, env = mats_of(f), LIGHTS[:2], ER.environment(ALL)
    r = RR.reflect(2, 1.0)
    hi, hi_st = both(renderer, hi_frame(f), r, env, mats, lights, abi.LIGHTS_COLOR)
    assert np.isfinite(hi).all()
    out, st = both(renderer, f, r, env, mats, lights, abi.LIGHTS_COLOR)
    assert same(out, ssaa_ref.resolve(hi, s)) and np.array_equal(st, hi_st)
    if prec == EXACT:
        want, want_st = hi_reference(name, s)
        assert same(out, ssaa_ref.resolve(want, s)) and np.array_equal(st, want_st)


# ---- 6. fast precision near the reference -------------------------------------------

def fast_deviation(rd, name, bounces):
    """(largest deviation, pixels left out, pixels): the fast composite against
    the reference replayed at the kernel's own per-layer step counts, on the
    pixels away from the miss boundary, where the layers traced must agree."""
    f, mats = fast_case(name)
    lights, env = [LIGHTS[0]], ER.environment(ALL)
    _, _, Sj, alive = G.own_layers(lambda r: both(rd, f, r, env, mats, lights, 0), bounces, 1.0)
    out, st = both(rd, f, RR.reflect(bounces, 1.0), env, mats, lights, 0)
    assert np.array_equal(st, Sj.sum(axis=2))
    return ER.fast_deviation(f, mats, lights, env, bounces, out, Sj, alive)


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name", ["C4", "C3", "REF"])
def test_fast_is_near_the_reference(renderer, name, bounces):
    """The fast composite with SKY | SUN | FOG against the reference replayed
    at the kernel's own per-layer step counts (one light, strength 1; the
    frames of test_gpu_reflect.py's fast test).  Pixels with a reached layer's
    reference d within 0.05 of max_dist are left out (there the hit / miss
    decision may flip), at most 2 % of the frame; on the rest the number of
    layers traced must agree.
    Measured on an MI355X (largest absolute deviation of a channel, bounces 1 /
    2; pixels left out): C4 1.413e-5 / 1.253e-4 (1 / 2), C3 7.21e-6 / 7.39e-6
    (2 / 2), REF 1.19e-6 / 1.01e-6 (2 / 2); the bound is 4 x the largest,
    FAST_BOUND = 5.01e-4."""
    dev, left_out, pixels = fast_deviation(renderer, name, bounces)
    print(f"{name} bounces {bounces}: largest deviation {dev:.3e}, {left_out} of {pixels} pixels "
          f"left out; bound {FAST_BOUND:.3e}")
    assert left_out <= ER.BOUNDARY_SHARE * pixels
    assert dev <= FAST_BOUND


# ---- 7. the C++ host program -------------------------------------------------------

def test_cpp_host_program_sky_and_fog_options(renderer, tmp_path):
    f = scenes.config("C3", 160, 90, precision=EXACT)                 # sdf_main's default
    scenes.set_view(f, scenes.orbit_view(180.0, 0.0))                 # frame 1 of 2: yaw 180
    f.params.output_format = abi.FORMAT_RGBA8
    env = scenes.sky(fog=(1.0, 4.0))
    want, _ = render(renderer, f, RR.reflect(2, 1.0), env, None, [f.light], 0, steps=False)
    plain, _ = render(renderer, f, RR.reflect(2, 1.0), None, None, [f.light], 0, steps=False)
    assert not same(want, plain)
    out = tmp_path / "f.ppm"
    r = sdf_main("--sky", "--fog", "1,4", "--reflect", "2", "160", "90", "2", out, "csg8")
    assert r.returncode == 0, r.stderr
    img = read_ppm(out)
    assert img.shape == (90, 160, 3)
    assert np.array_equal(img, want[::-1, :, :3])
    # fog alone in a colour of its own, the palette, no bounce
    env = scenes.sky(0, fog=(0.5, 3.0, (0.25, 0.5, 0.75)))
    pal = scenes.palette(8)
    fogged, _ = render(renderer, f, None, env, pal, [f.light], 0, steps=False)
    r = sdf_main("160", "90", "2", out, "csg8", "--palette", "--fog", "0.5,3,0.25,0.5,0.75")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_ppm(out), fogged[::-1, :, :3])
