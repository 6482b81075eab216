"""GPU tests of mirror reflections (sdf_render_reflect; include/sdf_abi.h
"Reflections"): the composite and its summed step counts bit for bit and on
every pixel against the CPU reference (tests/reflect_ref.py) in exact
precision, every single layer and weight plane with it; in both precisions the
composite against the composition of the kernel's own layers and weights;
within a measured bound against the reference in fast precision -- on every
dispatch path, for every output format, tiling, a schedule and supersampling.

Shape 37 x 23 (partial 8 x 8 tiles in x and y, a last block of 7 rows); the
supersampled cases use cases.SHAPES.  Every render writes into
buffers followed by sentinel rows, which must survive, and every case is
rendered with and without a steps buffer, which must not change the colours.
The SIX scenes run the generic kernel except where a test is about the path."""
import os

import numpy as np
import pytest

import lights_ref as LR
import materials_ref as MR
import reflect_ref as RR
import gpu_support as G
import ssaa_ref
from cases import frame_of, mats_of, mirror_scene
from gpu_support import SHAPES, bits, hi_frame, ndiff, read_ppm, rgba_of, same, sdf_main
from sdf3d_amd import abi, renderer as R, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
PRECS = [EXACT, FAST]
LIGHTS = LR.rig(8)
RIGS = [(1, 0), (3, abi.LIGHTS_COLOR)]
WEIGHT = abi.REFLECT_WEIGHT
# Fast precision's composite against the reference replayed at the kernel's
# per-layer step counts: the largest absolute deviation of a channel measured
# on an MI355X over C4 pose 0, C3 pose 2 (palette) and REF pose 0 (one
# material), bounces 1 and 2 (profiles/reflect_C4.json fast_deviation,
# DESIGN.md "Reflections"), and the bound asserted: 4 x that, the headroom
# test_gpu_materials.py's fast bound has.
FAST_MEASURED = 1.615e-4
FAST_BOUND = 4 * FAST_MEASURED


def shading(reflect, materials=None, lights=None, flags=0):
    return dict(reflect=reflect, materials=materials, lights=lights, light_flags=flags)


def render(rd, frame, reflect, materials=None, lights=None, flags=0, t=None, steps=True,
           schedule=None):
    """gpu_support.render with `reflect`: sdf_render_reflect; None with
    `materials`: sdf_render_materials."""
    return G.render(rd, frame, t, steps, schedule, **shading(reflect, materials, lights, flags))


def both(rd, frame, reflect, materials=None, lights=None, flags=0, t=None):
    return G.both(rd, frame, t, **shading(reflect, materials, lights, flags))


# ---- the reference, computed once per case and shared read-only ----------------

_REF = {}


def reference(name, pose, bounces, n, flags, strength=1.0):
    key = (name, pose, bounces, n, flags, strength)
    if key not in _REF:
        f = frame_of(name, pose)
        rgba, steps, w = RR.render(f, mats_of(f), bounces, strength, LIGHTS[:n], flags)
        assert np.isfinite(rgba).all(), key
        for a in (rgba, steps, w["C"], w["W"], w["alive"]):
            a.setflags(write=False)
        _REF[key] = (rgba, steps, w)
    return _REF[key]


def check_reference(rd, name, pose, bounces, n, flags, dispatch=None, layers=False):
    """Check 1: the exact composite and its summed steps are the reference's on
    every pixel; `layers`: so is every layer and every weight plane, with the
    layer's own steps."""
    f = frame_of(name, pose, EXACT, dispatch)
    want, want_st, w = reference(name, pose, bounces, n, flags)
    mats, lights = mats_of(f), LIGHTS[:n]
    out, st = both(rd, f, RR.reflect(bounces, 1.0), mats, lights, flags)
    print(f"differing words {ndiff(out, want)} of {out.size}; layer 1 alive "
          f"{w['alive'][:, :, 1].mean():.2f}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, want_st)
    if not layers:
        return
    lst = RR.layer_steps(w)
    for j in range(bounces + 1):
        cj, sj = both(rd, f, RR.reflect(bounces, 1.0, j), mats, lights, flags)
        assert same(cj, rgba_of(w["C"][:, :, j])), j
        assert np.array_equal(sj, lst[:, :, j]), j
        wj, wsj = both(rd, f, RR.reflect(bounces, 1.0, j, WEIGHT), mats, lights, flags)
        assert same(wj, rgba_of(w["W"][:, :, j])), j
        assert np.array_equal(wsj, lst[:, :, j]), j


# ---- 1. exact precision against the reference -----------------------------------

@pytest.mark.parametrize("n,flags", RIGS)
@pytest.mark.parametrize("bounces", [1, 3])
@pytest.mark.parametrize("name,pose", MR.FRAMES)
def test_exact_equals_reference(renderer, name, pose, bounces, n, flags):
    check_reference(renderer, name, pose, bounces, n, flags,
                    layers=(name, pose) in (("C4", 0), ("SIX", 2)))


@pytest.mark.parametrize("n,flags", RIGS)
def test_exact_mandelbulb_equals_reference(renderer, n, flags):
    check_reference(renderer, "C5", 0, 2, n, flags, layers=True)


# ---- 2. both precisions, from the kernel's own pieces ----------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,pose,n,flags", [("C4", 0, 2, abi.LIGHTS_COLOR), ("SIX", 2, 1, 0),
                                               ("C5", 0, 2, abi.LIGHTS_COLOR)])
def test_composite_is_the_fold_of_own_layers(renderer, name, pose, n, flags, prec):
    assert reference(name, pose, 3, n, flags, 0.75)[2]["alive"][:, :, 2].mean() > 0.02
    f = frame_of(name, pose, prec)
    mats, lights = mats_of(f), LIGHTS[:n]
    Cj, Wj, Sj, alive = G.own_layers(lambda r: both(renderer, f, r, mats, lights, flags), 3, 0.75)
    assert alive[:, :, 0].all() and (bits(Wj[:, :, 0]) == bits(np.ones(3, f32))).all()
    assert alive[:, :, 1].mean() > 0.02 and alive[:, :, 3].any()
    out, st = both(renderer, f, RR.reflect(3, 0.75), mats, lights, flags)
    want = RR.composite(Cj, Wj, alive, prec)
    print(f"differing words {ndiff(out, want)} of {out.size}")
    assert same(out, want), ndiff(out, want)
    assert np.array_equal(st, Sj.sum(axis=2))
    # layer 0 is sdf_render_materials's frame and steps
    m0, m0st = both(renderer, f, None, mats, lights, flags)
    assert same(rgba_of(Cj[:, :, 0]), m0) and np.array_equal(Sj[:, :, 0], m0st)


# ---- 3. degenerate cases ----------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("fmt", [abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8,
                                 abi.FORMAT_RGB32F])
def test_no_bounce_is_sdf_render_materials(renderer, fmt, prec):
    f = frame_of("C4", 0, prec)
    f.params.output_format = fmt
    mats, lights = mats_of(f), LIGHTS[:3]
    want, want_st = both(renderer, f, None, mats, lights, abi.LIGHTS_COLOR)
    for layer in (-1, 0):
        out, st = both(renderer, f, RR.reflect(0, 0.5, layer), mats, lights, abi.LIGHTS_COLOR)
        assert same(out, want) and np.array_equal(st, want_st)


@pytest.mark.parametrize("prec", PRECS)
def test_no_bounce_tiles_stream(renderer, prec):
    f = frame_of("C4", 0, prec)
    f.params.output_format = abi.FORMAT_TILES
    mats = [type(f.material).from_buffer_copy(f.material) for _ in range(f.scene.count)]
    kw = dict(lights=[LIGHTS[1]], materials=mats)
    G.tiles_streams(renderer, f, kw, dict(kw, reflect=(0, 1.0)))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,pose", [("C4", 0), ("SIX", 2), ("C5", 0)])
def test_nothing_reflected_is_no_bounce(renderer, name, pose, prec):
    """strength 0, and a table whose ref is 0 everywhere, end every path at
    layer 0: the reflect kernel's layer 0 is the materials kernel's pixel."""
    f = frame_of(name, pose, prec)
    mats, lights = mats_of(f), LIGHTS[:2]
    want, want_st = both(renderer, f, None, mats, lights, abi.LIGHTS_COLOR)
    out, st = both(renderer, f, RR.reflect(2, 0.0), mats, lights, abi.LIGHTS_COLOR)
    assert same(out, want) and np.array_equal(st, want_st)
    matte = [type(m).from_buffer_copy(m) for m in mats]
    for m in matte:
        m.ref[0] = m.ref[1] = m.ref[2] = 0.0
    want, want_st = both(renderer, f, None, matte, lights, abi.LIGHTS_COLOR)
    out, st = both(renderer, f, RR.reflect(2, 1.0), matte, lights, abi.LIGHTS_COLOR)
    assert same(out, want) and np.array_equal(st, want_st)
    one, _ = both(renderer, f, RR.reflect(2, 1.0, 1), matte, lights, abi.LIGHTS_COLOR)
    assert (bits(one[..., :3]) == 0).all() and (one[..., 3] == 1).all()


# ---- 4. dispatch paths -------------------------------------------------------------

PATHS = [("SIX", 2, abi.DISPATCH_UNCULLED), ("SIXH", 2, abi.DISPATCH_UNCULLED),
         ("C4", 0, abi.DISPATCH_GENERIC), ("C3", 2, abi.DISPATCH_UNCULLED),
         ("RJ", 2, abi.DISPATCH_AUTO), ("RJ", 2, abi.DISPATCH_GENERIC)]


@pytest.mark.parametrize("name,pose,dispatch", PATHS)
def test_paths_exact_equals_reference(renderer, name, pose, dispatch):
    w = reference(name, pose, 2, 3, abi.LIGHTS_COLOR)[2]
    assert w["alive"][:, :, 1].mean() > 0.1
    check_reference(renderer, name, pose, 2, 3, abi.LIGHTS_COLOR, dispatch, layers=name == "RJ")


@pytest.mark.parametrize("prec", PRECS)
def test_runtime_specialised_scene_compiles_one_kernel(renderer, prec):
    """A scene without a built-in variant: one run-time compiled reflect kernel
    serves every bounce count, layer, flag and strength (one more with step
    recording, one more with supersampling).  In exact precision its frame is
    the generic kernel's; in fast precision the two contract differently (as
    the materials kernels of this scene do), so the specialised kernel is
    checked against the composition of its own layers."""
    f = mirror_scene(prec, swapped=True)
    mats, lights = mats_of(f), LIGHTS[:2]
    jit = os.environ.get("SDF3D_JIT") != "0"
    count = renderer.lib.sdf_jit_count
    generic = f.copy()
    generic.params.dispatch = abi.DISPATCH_GENERIC
    want, want_st = both(renderer, generic, RR.reflect(2, 0.75), mats, lights)
    before = count()
    for b, s, layer, fl in ((2, 0.75, -1, 0), (1, 0.75, -1, 0), (4, 0.5, -1, 0), (3, 1.0, 2, 0),
                            (3, 1.0, 1, WEIGHT)):
        render(renderer, f, RR.reflect(b, s, layer, fl), mats, lights, steps=False)
        assert count() - before == (1 if jit else 0)
    out, _ = render(renderer, f, RR.reflect(2, 0.75), mats, lights, steps=False)
    assert prec == FAST or same(out, want)
    out2, st = render(renderer, f, RR.reflect(2, 0.75), mats, lights, steps=True)
    assert same(out2, out) and np.array_equal(st, want_st)
    assert count() - before == (2 if jit else 0)
    Cj, Wj, Sj, alive = G.own_layers(lambda r: both(renderer, f, r, mats, lights, 0), 2, 0.75)
    assert same(out, RR.composite(Cj, Wj, alive, prec)) and np.array_equal(st, Sj.sum(axis=2))
    assert count() - before == (2 if jit else 0)
    g = f.copy()
    g.params.width, g.params.height, g.params.samples = SHAPES[2][0], SHAPES[2][1], 2
    render(renderer, g, RR.reflect(2, 0.75), mats, lights, steps=False)
    render(renderer, g, RR.reflect(1, 0.25), mats, lights, steps=False)
    assert count() - before == (3 if jit else 0)


# ---- 5. formats, tilings, schedule, supersampling -----------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_formats_convert_the_composite(renderer, prec):
    f = frame_of("C4", 0, prec)
    mats, lights = mats_of(f), LIGHTS[:2]
    r = RR.reflect(2, 1.0)
    full, _ = render(renderer, f, r, mats, lights, abi.LIGHTS_COLOR, steps=False)
    plain, _ = render(renderer, f, None, mats, lights, abi.LIGHTS_COLOR, steps=False)
    assert np.abs(full - plain).max() > 0.1
    G.check_formats(renderer, f, full, **shading(r, mats, lights, abi.LIGHTS_COLOR))


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_term_streams_are_refused(renderer, fmt):
    import torch
    f = frame_of("C4", 0)
    f.params.output_format = fmt
    mats = [type(f.material).from_buffer_copy(f.material) for _ in range(f.scene.count)]
    if fmt == abi.FORMAT_TILES:
        out = torch.zeros(R.tiles_bytes(f.params.width, f.params.height), dtype=torch.uint8,
                          device=renderer.device)
    else:
        out = torch.zeros((f.params.height, f.params.width, 4), dtype=torch.float32,
                          device=renderer.device)
    for r in (RR.reflect(1, 1.0), RR.reflect(2, 1.0, 0), RR.reflect(0, 1.0, 0, WEIGHT)):
        with pytest.raises(abi.SdfError) as e:
            renderer.render(f, out=out, materials=mats, reflect=r)
        assert e.value.code == abi.SDF_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any(), "a refused render wrote to its buffer"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("world,shares", [(3, (1, 1)), (2, (1, 2))])
def test_tilings(renderer, world, shares, prec):
    f = frame_of("C3", 2, prec)
    mats, lights, flags = mats_of(f), LIGHTS[:2], abi.LIGHTS_COLOR
    r = RR.reflect(2, 1.0)
    G.check_tilings(renderer, f, world, shares, **shading(r, mats, lights, flags))


@pytest.mark.parametrize("prec", PRECS)
def test_scheduled(renderer, prec):
    f = frame_of("C3", 2, prec)
    mats, lights = mats_of(f), LIGHTS[:2]
    r = RR.reflect(2, 1.0)
    G.check_scheduled(renderer, f, **shading(r, mats, lights))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["C3", "SIX"])
def test_supersampled(renderer, name, s, prec):
    f = MR.frame_of(name, 2, prec, wh=SHAPES[s])
    if name == "SIX":
        f.params.dispatch = abi.DISPATCH_GENERIC
    f.params.samples = s
    mats, lights = mats_of(f), LIGHTS[:2]
    r = RR.reflect(2, 1.0)
    hi, hi_st = both(renderer, hi_frame(f), r, mats, lights, abi.LIGHTS_COLOR)
    assert np.isfinite(hi).all()
    plain, _ = render(renderer, hi_frame(f), None, mats, lights, abi.LIGHTS_COLOR, steps=False)
    assert np.abs(hi - plain).max() > 0.1
    out, st = both(renderer, f, r, mats, lights, abi.LIGHTS_COLOR)
    assert same(out, ssaa_ref.resolve(hi, s)) and np.array_equal(st, hi_st)


# ---- 6. fast precision near the reference -------------------------------------------

def fast_case(name):
    f = frame_of(name, {"C4": 0, "C3": 2, "REF": 0}[name], FAST)
    mats = (RR.materials_for(f) if name == "REF" else MR.palette_for(f))
    return f, mats


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name", ["C4", "C3", "REF"])
def test_fast_is_near_the_reference(renderer, name, bounces):
    """The fast composite against the reference replayed at the kernel's own
    per-layer step counts (one light, strength 1; C4 pose 0 and C3 pose 2 with
    the palette, whose folds have no hard decision after primitive 0, REF pose
    0 with one material on both primitives).  The number of layers traced must
    agree on every pixel, and no pixel is left out of the comparison.
    Measured on an MI355X (largest absolute deviation of a channel, bounces 1 /
    2): C4 1.788e-5 / 1.615e-4, C3 1.800e-5 / 1.860e-5, REF 7.99e-6 / 7.75e-6
    (a reflected ray magnifies the first hit's rounding: in the CPU prototype a
    1e-6 nudge of R moved a channel by up to 1.3e-4 on these frames); the bound
    is 4 x the largest, FAST_BOUND = 6.46e-4."""
    f, mats = fast_case(name)
    lights = [LIGHTS[0]]
    _, _, Sj, alive = G.own_layers(lambda r: both(renderer, f, r, mats, lights, 0), bounces, 1.0)
    out, st = both(renderer, f, RR.reflect(bounces, 1.0), mats, lights, 0)
    assert np.array_equal(st, Sj.sum(axis=2))
    force = np.zeros(alive.shape + (RR.FORCE,), dtype=np.int32)
    force[..., 0:2] = Sj
    g = f.copy()
    g.params.precision = EXACT
    want, _, w = RR.render(g, mats, bounces, 1.0, lights, 0, force=force)
    assert np.array_equal(alive, w["alive"]), \
        f"{int((alive != w['alive']).sum())} layers traced differ"
    assert alive[:, :, 1].mean() >= 0.1
    dev = float(np.abs(out.astype(np.float64) - want).max())
    print(f"{name} bounces {bounces}: largest deviation {dev:.3e} on all {alive[:, :, 0].size} "
          f"pixels; bound {FAST_BOUND:.3e}")
    assert dev <= FAST_BOUND


# ---- 7. the C++ host program -------------------------------------------------------

def test_cpp_host_program_reflect_option(renderer, tmp_path):
    f = scenes.config("C3", 160, 90, precision=EXACT)                 # sdf_main's default
    scenes.set_view(f, scenes.orbit_view(180.0, 0.0))                 # frame 1 of 2: yaw 180
    f.params.output_format = abi.FORMAT_RGBA8
    pal = scenes.palette(8)
    want, _ = render(renderer, f, RR.reflect(2, 1.0), pal, [f.light], 0, steps=False)
    plain, _ = render(renderer, f, None, pal, [f.light], 0, steps=False)
    assert not same(want, plain)
    out = tmp_path / "f.ppm"
    r = sdf_main("160", "90", "2", out, "csg8", "--palette", "--reflect", "2")
    assert r.returncode == 0, r.stderr
    img = read_ppm(out)
    assert img.shape == (90, 160, 3)
    assert np.array_equal(img, want[::-1, :, :3])
    # a strength, the option in front, and one material for every primitive
    half, _ = render(renderer, f, RR.reflect(1, 0.5), None, [f.light], 0, steps=False)
    r = sdf_main("--reflect", "1,0.5", "160", "90", "2", out, "csg8")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_ppm(out), half[::-1, :, :3])
