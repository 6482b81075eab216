"""GPU tests of multi-light rendering (sdf_render_lights; include/sdf_abi.h
"Lights"): an L-light frame is the composition of its lights' single-light
shading terms in the contract's order (tests/lights_ref.py), bit for bit and
on every pixel -- against the CPU oracle in exact precision, against the
build's own single-light renders in both precisions -- on every dispatch
path, for every output format, tiling, a schedule and supersampling, with the
step counts (primary, sum of the lights' shadow counts).

Shape 37 x 23 (partial 8 x 8 tiles in x and y, a last block of 7 rows); the
supersampled cases use cases.SHAPES.  Every render writes into
buffers followed by sentinel rows, which must survive, and every case is
rendered with and without a steps buffer, which must not change the colours."""
import os

import numpy as np
import pytest

import lights_ref as LR
import oracle
import gpu_support as G
import ssaa_ref
from cases import specialised_scene
from gpu_support import SHAPES, hi_frame, ndiff, own_light, read_ppm, same, sdf_main
from parity import quantize
from sdf3d_amd import abi, scenes

pytestmark = pytest.mark.gpu

PRECS = [abi.PRECISION_EXACT, abi.PRECISION_FAST]
FLAGS = [0, abi.LIGHTS_COLOR]
LIGHTS = LR.rig(8)


def frame_of(cfg, pose, prec=abi.PRECISION_EXACT, wh=LR.SHAPE):
    return scenes.config(cfg, *wh, precision=prec, pose=pose)


def render(rd, frame, lights=None, flags=0, t=None, steps=True, schedule=None):
    """gpu_support.render with `lights`: sdf_render_lights."""
    return G.render(rd, frame, t, steps, schedule, lights=lights, light_flags=flags)


def both(rd, frame, lights=None, flags=0, t=None):
    return G.both(rd, frame, t, lights=lights, light_flags=flags)


# ---- references, computed once and shared read-only ---------------------------

_ORACLE = {}


def oracle_light(cfg, pose, i):
    """(terms, steps) of the oracle for (cfg, pose) under rig light i alone."""
    key = (cfg, pose, i)
    if key not in _ORACLE:
        g = LR.with_light(frame_of(cfg, pose), LIGHTS[i])
        terms = oracle.render_terms(g)
        _, steps = oracle.render(g)
        assert np.isfinite(terms).all(), key
        terms.setflags(write=False)
        steps.setflags(write=False)
        _ORACLE[key] = (terms, steps)
    return _ORACLE[key]


def own_compose(rd, f, lights, flags, key=None):
    """(colour, steps) the contract gives from the build's own single-light
    renders of `f`."""
    parts = [own_light(rd, f, l, None if key is None else (*key, i))
             for i, l in enumerate(lights)]
    want = LR.compose(f, [p[0] for p in parts], lights, flags, f.params.precision,
                      specs=[p[1] for p in parts])
    st = parts[0][2].copy()
    st[..., 1] = sum(p[2][..., 1] for p in parts)
    for p in parts[1:]:
        assert np.array_equal(p[2][..., 0], parts[0][2][..., 0])
        assert same(p[0][..., 0], parts[0][0][..., 0])      # ao
    return want, st


def check_against_own(rd, f, lights, flags, key=None, t=None):
    want, want_st = own_compose(rd, f, lights, flags, key)
    out, st = both(rd, f, lights, flags)
    print(f"differing words {ndiff(out, want)} of {out.size}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, want_st)
    return out, st


# ---- 1. exact precision against the oracle --------------------------------------

@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("cfg,pose", LR.FRAMES)
def test_exact_equals_composed_oracle(renderer, cfg, pose, n, flags):
    f = frame_of(cfg, pose)
    parts = [oracle_light(cfg, pose, i) for i in range(n)]
    want = LR.compose(f, [p[0] for p in parts], LIGHTS[:n], flags, abi.PRECISION_EXACT)
    want_st = parts[0][1].copy()
    want_st[..., 1] = sum(p[1][..., 1] for p in parts)
    out, st = both(renderer, f, LIGHTS[:n], flags)
    print(f"differing words {ndiff(out, want)} of {out.size}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, want_st)


# ---- 2. both precisions against the build's own single-light renders ------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("cfg,pose", LR.FRAMES)
def test_equals_own_single_light_renders(renderer, cfg, pose, n, flags, prec):
    oracle_light(cfg, pose, n - 1)             # the inputs are finite
    f = frame_of(cfg, pose, prec)
    check_against_own(renderer, f, LIGHTS[:n], flags, key=(cfg, pose, prec))


# ---- 3. one plain light is sdf_render itself --------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("fmt", [abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8,
                                 abi.FORMAT_RGB32F, abi.FORMAT_SHADE32F])
def test_one_plain_light_is_sdf_render(renderer, fmt, prec):
    f = LR.with_light(frame_of("C3", 2, prec), LIGHTS[1])
    f.params.output_format = fmt
    base, base_st = both(renderer, f)
    g = LR.with_light(f, LIGHTS[4])            # frame.light is ignored
    one, one_st = both(renderer, g, [LIGHTS[1]], 0)
    assert same(one, base) and np.array_equal(one_st, base_st)
    if prec == abi.PRECISION_EXACT and fmt == abi.FORMAT_RGBA32F:
        assert same(base, oracle.render(f)[0])


@pytest.mark.parametrize("prec", PRECS)
def test_one_plain_light_tiles_stream(renderer, prec):
    import torch
    f = LR.with_light(frame_of("C3", 2, prec), LIGHTS[1])
    f.params.output_format = abi.FORMAT_TILES
    _, b, _ = G.tiles_streams(renderer, f, {}, dict(lights=[LIGHTS[1]]))
    g = f.copy()
    g.params.output_format = abi.FORMAT_RGBA32F
    frame = renderer.tiles_decode(b, 1, b.numel(), f.params.width, f.params.height)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), render(renderer, g, steps=False)[0])


# ---- 4. kernel paths ------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dispatch", [abi.DISPATCH_GENERIC, abi.DISPATCH_UNCULLED])
def test_generic_kernel_paths(renderer, dispatch, prec):
    oracle_light("C3", 2, 2)
    f = frame_of("C3", 2, prec)
    f.params.dispatch = dispatch
    out, _ = check_against_own(renderer, f, LIGHTS[:3], abi.LIGHTS_COLOR)
    if prec == abi.PRECISION_EXACT:
        parts = [oracle_light("C3", 2, i)[0] for i in range(3)]
        assert same(out, LR.compose(f, parts, LIGHTS[:3], abi.LIGHTS_COLOR))


@pytest.mark.parametrize("prec", PRECS)
def test_runtime_specialised_scene(renderer, prec):
    f = specialised_scene(prec)
    ref = [oracle.render_terms(LR.with_light(f, l)) for l in LIGHTS[:3]]
    assert all(np.isfinite(r).all() for r in ref)
    want, want_st = own_compose(renderer, f, LIGHTS[:3], 0)   # compiles the plain kernels
    jit = os.environ.get("SDF3D_JIT") != "0"
    count = renderer.lib.sdf_jit_count
    before = count()
    for flags in FLAGS:                        # one kernel serves the flag and every L
        for n in (3, 2):
            out, _ = render(renderer, f, LIGHTS[:n], flags, steps=False)
            assert count() - before == (1 if jit else 0)
    out, _ = render(renderer, f, LIGHTS[:3], 0, steps=False)
    assert same(out, want)
    out, st = render(renderer, f, LIGHTS[:3], 0, steps=True)
    assert same(out, want) and np.array_equal(st, want_st)
    assert count() - before == (2 if jit else 0)
    g = f.copy()
    g.params.width, g.params.height, g.params.samples = SHAPES[2][0], SHAPES[2][1], 2
    render(renderer, g, LIGHTS[:3], 0, steps=False)
    render(renderer, g, LIGHTS[:2], abi.LIGHTS_COLOR, steps=False)
    assert count() - before == (3 if jit else 0)
    if prec == abi.PRECISION_EXACT:
        assert same(want, LR.compose(f, ref, LIGHTS[:3], 0))


# ---- 5. output formats ----------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("flags", FLAGS)
def test_formats_convert_the_colour(renderer, flags, prec):
    oracle_light("C4", 0, 2)
    f = frame_of("C4", 0, prec)
    full, _ = render(renderer, f, LIGHTS[:3], flags, steps=False)
    G.check_formats(renderer, f, full, lights=LIGHTS[:3], light_flags=flags)


# ---- 6. supersampling -----------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("cfg,pose", [("C3", 2), ("C5", 3)])
def test_supersampled(renderer, cfg, pose, s, prec):
    f = frame_of(cfg, pose, prec, wh=SHAPES[s])
    f.params.samples = s
    assert np.isfinite(oracle.render(hi_frame(f))[0]).all()
    for flags in FLAGS:
        hi, hi_st = both(renderer, hi_frame(f), LIGHTS[:2], flags)
        out, st = both(renderer, f, LIGHTS[:2], flags)
        assert same(out, ssaa_ref.resolve(hi, s)) and np.array_equal(st, hi_st)


# ---- 7. tilings -----------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("world,shares", [(3, (1, 1)), (2, (1, 2))])
def test_tilings(renderer, world, shares, prec):
    oracle_light("C3", 2, 1)
    f = frame_of("C3", 2, prec)
    G.check_tilings(renderer, f, world, shares, lights=LIGHTS[:2], light_flags=abi.LIGHTS_COLOR)


# ---- 8. schedule ----------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_scheduled(renderer, prec):
    oracle_light("C3", 2, 1)
    f = frame_of("C3", 2, prec)

    def one_plain_light(sch):      # under the schedule: sdf_render_scheduled itself
        one, _ = render(renderer, LR.with_light(f, LIGHTS[0]), steps=False, schedule=sch)
        two, _ = render(renderer, f, [LIGHTS[0]], 0, steps=False, schedule=sch)
        assert same(one, two)
    G.check_scheduled(renderer, f, after=one_plain_light, lights=LIGHTS[:2], light_flags=0)


# ---- 9. the C++ host program ----------------------------------------------------------

def test_cpp_host_program_lights_argument(renderer, tmp_path):
    f = scenes.config("C3", 160, 90, precision=abi.PRECISION_EXACT)   # sdf_main's default
    scenes.set_view(f, scenes.orbit_view(180.0, 0.0))                 # frame 1 of 2: yaw 180
    # sdf_main's lights: the first carries the reference ambient, a light
    # without r,g,b is white
    lights = LR.rig(2)
    lights[0].ambient, lights[1].ambient = f.light.ambient, 0.0
    for c in range(3):
        lights[0].color[c] = 1.0
    terms = [oracle.render_terms(LR.with_light(f, l)) for l in lights]
    assert all(np.isfinite(t).all() for t in terms)
    f.params.output_format = abi.FORMAT_RGBA8
    want, _ = render(renderer, f, lights, abi.LIGHTS_COLOR, steps=False)
    assert same(want, quantize(LR.compose(f, terms, lights, abi.LIGHTS_COLOR), abi.FORMAT_RGBA8))
    out = tmp_path / "f.ppm"
    r = sdf_main("160", "90", "2", out, "csg8", "1", "-4,3,3;-2,0.6,1,0.25,0.5,1")
    assert r.returncode == 0, r.stderr
    img = read_ppm(out)
    assert img.shape == (90, 160, 3)
    assert np.array_equal(img, want[::-1, :, :3])
