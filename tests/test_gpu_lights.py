"""GPU tests of multi-light rendering (sdf_render_lights; include/sdf_abi.h
"Lights"): an L-light frame is the composition of its lights' single-light
shading terms in the contract's order (tests/lights_ref.py), bit for bit and
on every pixel -- against the CPU oracle in exact precision, against the
build's own single-light renders in both precisions -- on every dispatch
path, for every output format, tiling, a schedule and supersampling, with the
step counts (primary, sum of the lights' shadow counts).

Shape 37 x 23 (partial 8 x 8 tiles in x and y, a last block of 7 rows); the
supersampled cases use test_gpu_ssaa.py's shapes.  Every render writes into
buffers followed by sentinel rows, which must survive, and every case is
rendered with and without a steps buffer, which must not change the colours."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lights_ref as LR
import oracle
import ssaa_ref
from parity import quantize
from sdf3d_amd import abi, renderer as R, scenes
from test_gpu_ssaa import (FILL, SHAPES, _guarded, _sentinel, bits, hi_frame, owned_row_index,
                           read_ppm, same)

pytestmark = pytest.mark.gpu

PRECS = [abi.PRECISION_EXACT, abi.PRECISION_FAST]
FLAGS = [0, abi.LIGHTS_COLOR]
LIGHTS = LR.rig(8)


def frame_of(cfg, pose, prec=abi.PRECISION_EXACT, wh=LR.SHAPE):
    return scenes.config(cfg, *wh, precision=prec, pose=pose)


def render(rd, frame, lights=None, flags=0, t=None, steps=True, schedule=None):
    """Renderer.render (with `lights`: sdf_render_lights) into sentinel-filled
    buffers with guard rows behind them, which are checked.  NumPy arrays."""
    import torch
    p = frame.params
    rows = R.buffer_rows(p.height, t)
    shape = (rows, p.width, R.channels(p.output_format))
    buf = _guarded(torch, rd.device, shape, R.torch_dtype(p.output_format))
    sshape = R.steps_shape(frame, t)
    sbuf = _guarded(torch, rd.device, sshape, torch.int32) if steps else None
    rd.render(frame, t, out=buf[:rows], steps=sbuf[:sshape[0]] if steps else False,
              schedule=schedule, lights=lights, light_flags=flags)
    torch.cuda.synchronize()
    assert _sentinel(torch, buf[rows:]), "colour buffer: rows past the end were written"
    if steps:
        assert _sentinel(torch, sbuf[sshape[0]:]), "steps buffer: rows past the end were written"
    return buf[:rows].cpu().numpy(), (sbuf[:sshape[0]].cpu().numpy() if steps else None)


def both(rd, frame, lights=None, flags=0, t=None):
    """Without a steps buffer (the shortcuts active) and with one: the same
    colours.  Returns (rgba, steps)."""
    a, _ = render(rd, frame, lights, flags, t, steps=False)
    b, st = render(rd, frame, lights, flags, t, steps=True)
    assert same(a, b), "renders with and without a steps buffer differ"
    return a, st


def ndiff(a, b):
    a, b = (np.ascontiguousarray(v).view(np.uint32) for v in (a, b))
    return int((a != b).sum())


# ---- references, computed once and shared read-only ---------------------------

_ORACLE = {}
_OWN = {}


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


def spec_frame(f):
    """`f` with material amb = dif = 0 and ref = 1: its colour is spec exactly
    (fma(spec, 1, fma(dif, 0, 0 * ao)) in fast precision)."""
    g = f.copy()
    for c in range(3):
        g.material.amb[c], g.material.dif[c], g.material.ref[c] = 0.0, 0.0, 1.0
    return g


def own_light(rd, f, light, key=None):
    """(terms, spec, steps) of the build's own single-light renders of `f`
    under `light`: terms from SDF_FORMAT_SHADE32F, spec from the colour of
    spec_frame, the steps of the plain render."""
    if key is not None and key in _OWN:
        return _OWN[key]
    g = LR.with_light(f, light)
    g.params.output_format = abi.FORMAT_SHADE32F
    terms, steps = both(rd, g)
    h = spec_frame(LR.with_light(f, light))
    spec = both(rd, h)[0][..., 0].copy()
    assert np.isfinite(terms).all() and np.isfinite(spec).all()
    if f.params.precision == abi.PRECISION_EXACT:
        assert same(spec, LR.spec_exact(terms[..., 2], f.material.shininess))
    for a in (terms, spec, steps):
        a.setflags(write=False)
    if key is not None:
        _OWN[key] = (terms, spec, steps)
    return terms, spec, steps


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
    w, h = f.params.width, f.params.height
    # zeroed buffers: a stream has alignment gaps the encoder does not write
    a, b = (torch.zeros(R.tiles_bytes(w, h), dtype=torch.uint8, device=renderer.device)
            for _ in range(2))
    renderer.render(f, out=a)
    renderer.render(f, out=b, lights=[LIGHTS[1]])
    torch.cuda.synchronize()
    n = R.tiles_stream_bytes(a)
    assert n == R.tiles_stream_bytes(b) and n > abi.TILES_HEADER_BYTES
    assert torch.equal(a[:n], b[:n])
    g = f.copy()
    g.params.output_format = abi.FORMAT_RGBA32F
    frame = renderer.tiles_decode(b, 1, b.numel(), w, h)
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


def specialised_scene(prec):
    """plane, torus, box in hard union: no built-in variant, so
    SDF_DISPATCH_AUTO compiles its kernel at run time (hipRTC).  As
    test_gpu_ssaa.py's unmatched_scene, but a signature of its own (the
    primitives in another order): that test counts its scene's compilations."""
    f = frame_of("C3", 2, prec)
    f.scene.count = 3
    scenes._prim(f.scene, 1, abi.PRIM_TORUS, abi.OP_UNION, 0.0, 0.4, 0.1, 0.0, 0.2, 0.06)
    scenes._prim(f.scene, 2, abi.PRIM_BOX, abi.OP_UNION, 0.0, -0.4, 0.15, 0.0, 0.15, 0.15, 0.15)
    return f


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
    for fmt in (abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        g = f.copy()
        g.params.output_format = fmt
        out, _ = both(renderer, g, LIGHTS[:3], flags)
        assert same(out, quantize(full, fmt)), fmt


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
    w, h = f.params.width, f.params.height
    lights, flags = LIGHTS[:2], abi.LIGHTS_COLOR
    whole, whole_st = both(renderer, f, lights, flags)
    seen = np.zeros(h, dtype=int)
    for rank in range(world):
        t = R.tiling(rank, world, 8, shares=shares)
        rows = owned_row_index(h, t)
        assert len(rows) == R.owned_rows(h, t)
        seen[rows] += 1
        out, st = both(renderer, f, lights, flags, t)
        assert out.shape == (len(rows), w, 4)
        assert same(out, whole[rows]) and np.array_equal(st, whole_st[rows])
        tf = R.tiling(rank, world, 8, frame_rows=True, shares=shares)
        fr, fr_st = both(renderer, f, lights, flags, tf)
        other = np.setdiff1d(np.arange(h), rows)
        assert same(fr[rows], whole[rows]) and np.array_equal(fr_st[rows], whole_st[rows])
        assert (bits(fr[other]) == FILL).all() and (bits(fr_st[other]) == FILL).all()
    assert (seen == 1).all()


# ---- 8. schedule ----------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_scheduled(renderer, prec):
    oracle_light("C3", 2, 1)
    f = frame_of("C3", 2, prec)
    ref, ref_st = render(renderer, f, LIGHTS[:2], 0, steps=True)
    sch = renderer.schedule(f.params.height, period=1)
    try:
        for _ in range(3):
            out, st = render(renderer, f, LIGHTS[:2], 0, steps=True, schedule=sch)
            assert same(out, ref) and np.array_equal(st, ref_st)
        assert sorted(sch.order()) == list(range((f.params.height + 7) // 8))
        # one plain light under the schedule: sdf_render_scheduled itself
        one, _ = render(renderer, LR.with_light(f, LIGHTS[0]), steps=False, schedule=sch)
        two, _ = render(renderer, f, [LIGHTS[0]], 0, steps=False, schedule=sch)
        assert same(one, two)
    finally:
        sch.close()


# ---- 9. the C++ host program ----------------------------------------------------------

def test_cpp_host_program_lights_argument(renderer, tmp_path):
    exe = Path(__file__).resolve().parent.parent / "sdf3d_amd" / "bin" / "sdf_main"
    assert exe.exists(), "build() must produce sdf3d_amd/bin/sdf_main"
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
    r = subprocess.run([str(exe), "160", "90", "2", str(out), "csg8", "1",
                        "-4,3,3;-2,0.6,1,0.25,0.5,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = read_ppm(out)
    assert img.shape == (90, 160, 3)
    assert np.array_equal(img, want[::-1, :, :3])
