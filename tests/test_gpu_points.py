"""GPU tests of shading at caller-supplied points (sdf_shade_points;
include/sdf_abi.h "Points").  In exact precision, bit for bit: the hit points of
a frame, formed on the host, against sdf_render_materials's pixels, shadow
counts and occlusion term on every dispatch path; points off the surface, a
lift, supplied normals and no eye, under 1, 3 and 8 lights, against the CPU
reference (tests/points_ref.c); each output alone against the call with all of
them; short point lists against the prefix of the long one.  Fast precision
within a measured bound of the reference replayed at the kernel's own shadow
counts.  End to end: Renderer.bake on a mesh, and the host program's
--mesh-colors.

The point set is the 37 x 23 frame's 851 hit points: 13 full waves and 19 lanes.
Every call writes into fenced buffers (points_ref.kernel_shade): the 64 guard rows
in front of every output and those behind it must survive."""
import numpy as np
import pytest

import materials_ref as MR
import oracle
import points_ref as PR
from cases import LIGHTS
from gpu_support import both as frame_both
from gpu_support import ndiff, same, sdf_main
from gpu_support import render as frame_render
from points_ref import FAST_CASES, OUTS, fast_deviation, mats_of, the_frame
from points_ref import frame_hits as hit_points
from points_ref import kernel_shade as shade
from sdf3d_amd import abi, meshio, renderer as R, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
A, G, U = abi.DISPATCH_AUTO, abi.DISPATCH_GENERIC, abi.DISPATCH_UNCULLED
CLR = abi.LIGHTS_COLOR
W, H = MR.SHAPE
N = W * H

# Fast precision against the reference replayed at the kernel's own shadow
# counts, on all 851 hit points of C4 pose 0, C3 pose 2 (palette) and REF pose
# 0, three lights with colours: the largest absolute deviation of rgba, ao and
# shadow measured on an MI355X (C4: rgba 1.07e-6, ao 4.77e-7, shadow 9.50e-6;
# C3: 1.55e-6, 4.77e-7, 2.253e-5; REF: 1.19e-6, 0, 8.12e-6;
# profiles/points_C4.json fast_deviation, DESIGN.md "shade_points"), and the
# bound asserted: 4 x that, the headroom every other fast bound in tests/ has.
FAST_MEASURED = 2.253e-5
FAST_BOUND = 4 * FAST_MEASURED
# `material` likewise, where no hard decision of the fold is closer than
# materials_ref.GAP (test_gpu_materials.FAST_BOUND's construction; here the
# kernel and the reference fold at the same point, so every point counts): C4 0,
# C3 8.941e-8, REF 0
FAST_MATERIAL_MEASURED = 8.941e-8
FAST_MATERIAL_BOUND = 4 * FAST_MATERIAL_MEASURED


# ---- 1. identity with the render -----------------------------------------------------------

# (frame, pose, dispatch, a palette instead of the frame's one material)
IDENTITY = [("C4", 0, A, False), ("C3", 2, A, True), ("REF", 0, A, True), ("C5", 0, A, False),
            ("C3", 2, G, True), ("C3", 2, U, True), ("PJ", 2, A, True)]


@pytest.mark.parametrize("name,pose,dispatch,pal", IDENTITY)
def test_hit_points_shade_to_the_frame(renderer, name, pose, dispatch, pal):
    """rgba, steps and ao at the frame's hit points are sdf_render_materials's
    pixels, its shadow counts and SHADE32F's channel 0, bit for bit."""
    f = the_frame(name, pose, EXACT, dispatch)
    mats = mats_of(f, pal)
    want, want_st = frame_both(renderer, f, materials=mats, lights=[f.light])
    P, eye = hit_points(renderer, name, pose)
    got = shade(renderer, f, P, eye=eye, materials=mats)
    print(f"differing words: rgba {ndiff(got.rgba, want.reshape(N, 4))} of {4 * N}, "
          f"steps {int((got.steps[:, 0] != want_st.reshape(N, 2)[:, 1]).sum())} of {N}")
    assert same(got.rgba, want.reshape(N, 4))
    assert np.array_equal(got.steps[:, 0], want_st.reshape(N, 2)[:, 1])
    g = f.copy()
    g.params.output_format = abi.FORMAT_SHADE32F
    terms, _ = frame_render(renderer, g, steps=False)
    terms = terms.reshape(N, -1)
    print(f"differing words: ao {ndiff(got.ao, terms[:, 0])} of {N}")
    assert same(got.ao, np.ascontiguousarray(terms[:, 0]))
    # dif = clamp(N . incident, 0, 1) sh: where it is above 0 the factor is
    assert (got.shadow[terms[:, 1] > 0, 0] > 0).all()


def test_the_run_time_compiled_kernel_is_counted(renderer):
    f = the_frame("PJC", 2)
    P, eye = hit_points(renderer, "C3", 2)
    before = renderer.lib.sdf_jit_count()
    a = shade(renderer, f, P[:130], eye=eye, materials=mats_of(f), outs=("rgba",))
    assert renderer.lib.sdf_jit_count() == before + 1
    b = shade(renderer, f, P[:130], eye=eye, materials=mats_of(f), outs=("rgba",))
    assert renderer.lib.sdf_jit_count() == before + 1 and same(a.rgba, b.rgba)
    g = f.copy()
    g.params.dispatch = G
    c = shade(renderer, g, P[:130], eye=eye, materials=mats_of(f), outs=("rgba",))
    assert renderer.lib.sdf_jit_count() == before + 1 and same(a.rgba, c.rgba)


# ---- 2. against the reference: off the surface, lights, lift, normals, no eye -----------------

def lattice():
    """The 5 x 5 x 5 lattice around C4: 125 points, one full wave and 61 lanes,
    most of them off the surface, some inside the solid."""
    x = np.linspace(-1.0, 1.0, 5, dtype=f32)
    y = np.linspace(0.02, 0.9, 5, dtype=f32)
    g = np.stack(np.meshgrid(x, y, x, indexing="ij"), axis=-1).reshape(-1, 3)
    assert g.shape == (125, 3)
    return np.ascontiguousarray(g, dtype=f32)


def check_exact(got, ref, what):
    for k in ("rgba", "shadow", "material", "steps", "ao"):
        a, b = getattr(got, k), getattr(ref, k)
        d = ndiff(a, b)
        print(f"{what}: {k} differing words {d} of {a.size}")
    for k in ("rgba", "shadow", "material", "steps", "ao"):
        assert same(getattr(got, k), getattr(ref, k)), (what, k)


@pytest.mark.parametrize("flags", [0, CLR], ids=["plain", "colour"])
@pytest.mark.parametrize("nl", [1, 3, 8])
def test_lattice_equals_the_reference(renderer, nl, flags):
    f = the_frame("C4", 0)
    mats = mats_of(f)
    Q = lattice()
    eye = (1.5, 1.0, 2.0)
    rng = np.random.default_rng(nl)
    given = (rng.standard_normal(Q.shape) * 0.7).astype(f32)    # not unit: used as given
    cases = {"eye": dict(eye=eye), "lift, no eye": dict(lift=0.05),
             "normals, lift, eye": dict(normals=given, lift=0.02, eye=eye)}
    for what, kw in cases.items():
        got = shade(renderer, f, Q, lights=LIGHTS[:nl], flags=flags, materials=mats, **kw)
        ref = PR.shade(f, Q, lights=LIGHTS[:nl], light_flags=flags, materials=mats, **kw)
        check_exact(got, ref, f"L={nl} {what}")


def test_mandelbulb_lattice_equals_the_reference(renderer):
    f = the_frame("C5", 0)
    Q = lattice()[::2]
    m = scenes.palette(3)[2:]
    got = shade(renderer, f, Q, lights=LIGHTS[:3], flags=CLR, materials=m, eye=(0.0, 1.5, 2.0),
                lift=0.01)
    ref = PR.shade(f, Q, lights=LIGHTS[:3], light_flags=CLR, materials=m, eye=(0.0, 1.5, 2.0),
                   lift=0.01)
    check_exact(got, ref, "C5")


# ---- 3. what is asked for, and how many ------------------------------------------------------

_ALL = {}


def all_outputs(rd):
    """Every output of the 851-point call on C3 with its palette, 3 lights."""
    if not _ALL:
        f = the_frame("C3", 2)
        P, eye = hit_points(rd, "C3", 2)
        _ALL["r"] = (f, P, eye, shade(rd, f, P, eye=eye, lights=LIGHTS[:3], flags=CLR,
                                     materials=mats_of(f)))
    return _ALL["r"]


@pytest.mark.parametrize("only", OUTS)
def test_each_output_alone_has_its_bits(renderer, only):
    f, P, eye, full = all_outputs(renderer)
    got = shade(renderer, f, P, eye=eye, lights=LIGHTS[:3], flags=CLR, materials=mats_of(f),
                outs=(only,))
    assert same(getattr(got, only), getattr(full, only)), ndiff(getattr(got, only),
                                                                getattr(full, only))
    assert all(getattr(got, k) is None for k in OUTS if k != only)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_short_lists_are_the_prefix(renderer, n):
    f, P, eye, full = all_outputs(renderer)
    got = shade(renderer, f, P[:n], eye=eye, lights=LIGHTS[:3], flags=CLR, materials=mats_of(f))
    for k in OUTS:
        assert same(getattr(got, k), getattr(full, k)[:n]), k


def test_renderer_shade_points_is_the_abi_call(renderer):
    import torch
    f, P, eye, full = all_outputs(renderer)
    dev = lambda a: torch.from_numpy(np.array(a, dtype=f32)).to(renderer.device)
    s = renderer.shade_points(f, dev(P), eye=eye, lights=LIGHTS[:3], light_flags=CLR,
                              materials=mats_of(f), ao=True, shadow=True, material=True,
                              steps=True)
    torch.cuda.synchronize()
    assert isinstance(s, R.Shade)
    for k in OUTS:
        assert same(getattr(s, k).cpu().numpy(), getattr(full, k)), k
    s = renderer.shade_points(f, dev(P[:70]))
    torch.cuda.synchronize()
    assert s.rgba.shape == (70, 4) and s.ao is None and s.shadow is None and s.steps is None
    assert torch.isfinite(s.rgba).all() and (s.rgba[:, 3] == 1).all()
    e = renderer.shade_points(f, dev(P[:0]), ao=True)
    assert e.rgba.shape == (0, 4) and e.ao.shape == (0,)
    with pytest.raises(ValueError):
        renderer.shade_points(f, dev(P), rgba=False)


# ---- 4. fast precision ------------------------------------------------------------------------

@pytest.mark.parametrize("name,pose,pal", FAST_CASES)
def test_fast_within_the_measured_bound(renderer, name, pose, pal):
    """Every point counts: the reference is replayed at the kernel's own shadow
    counts, so no break-point flip needs excusing."""
    dev, far = fast_deviation(renderer, name, pose, pal)
    print(f"fast deviation {name}: " + ", ".join(f"{k} {v:.4e}" for k, v in dev.items()) +
          f"; material on {far} of {N} points")
    assert far >= 0.95 * N
    assert max(dev["rgba"], dev["ao"], dev["shadow"]) <= FAST_BOUND, dev
    assert dev["material"] <= FAST_MATERIAL_BOUND, dev


# ---- 5. end to end ------------------------------------------------------------------------------

# 16^3 cells over the two spheres on top of C4 (439 vertices): with the default
# lift no lifted vertex has a negative reference distance.  (The whole scene at
# 16^3 does: its cells are wider than the torus' tube, and a lift of one cell
# diagonal from a concave junction ends inside the neighbouring primitive.)
BAKE_ORIGIN, BAKE_CELL, BAKE_N = (0.05, 0.45, -0.35), 0.025, 16


def test_bake_colours_every_vertex(renderer):
    import torch
    f = the_frame("C4", 0)
    m = renderer.mesh(f, BAKE_ORIGIN, BAKE_CELL, BAKE_N, normal=True)
    col = renderer.bake(f, m, BAKE_CELL, eye=(1.5, 1.0, 2.0), materials=mats_of(f))
    torch.cuda.synchronize()
    nv = m.verts.shape[0]
    assert nv > 300 and col.shape == (nv, 4) and col.dtype == torch.float32
    col = col.cpu().numpy()
    assert np.isfinite(col).all() and (col[:, 3] == 1).all() and (col[:, :3] >= 0).all()
    assert len(np.unique(col[:, :3].view(np.uint32), axis=0)) > nv // 2
    # the default lift is the cell diagonal, and it puts every vertex outside
    lift = f32(np.sqrt(3.0 * BAKE_CELL * BAKE_CELL))
    v, n = m.verts.cpu().numpy(), m.normal.cpu().numpy()
    lifted = (v + (n * lift).astype(f32)).astype(f32)
    d = np.array([oracle.scene_sdf(f.scene, *map(float, p)) for p in lifted])
    assert (d >= 0).all(), float(d.min())
    want = renderer.shade_points(f, m.verts, normals=m.normal, eye=(1.5, 1.0, 2.0),
                                 lift=float(lift), materials=mats_of(f)).rgba
    torch.cuda.synchronize()
    assert same(want.cpu().numpy(), col)
    # without normals on the mesh the kernel takes its own
    bare = renderer.bake(f, R.Mesh(m.verts, m.tris, None, None, m.counts), BAKE_CELL,
                         eye=(1.5, 1.0, 2.0), materials=mats_of(f))
    torch.cuda.synchronize()
    assert same(bare.cpu().numpy(), col)


def test_cpp_host_program_mesh_colors(renderer, tmp_path):
    """sdf_main --palette --mesh FILE.ply --mesh-colors writes the mesh Renderer.mesh
    gives for its csg8 scene (C3's) with the colours Renderer.bake gives, as
    bytes, which read_ply reads back."""
    import math
    import torch
    ply = tmp_path / "m.ply"
    n = BAKE_N
    lo = [float(x) for x in BAKE_ORIGIN]
    hi = [a + BAKE_CELL * n for a in lo]
    r = sdf_main("--palette", "--mesh", ply, "--mesh-colors", "--grid",
                 ",".join(repr(x) for x in (*lo, *hi)) + f",{n}", "64", "36", "1",
                 tmp_path / "f.ppm", "csg8")
    assert r.returncode == 0, r.stderr
    # the grid the program makes of the box: its extent over n in fp64, rounded once
    cell = tuple(float(f32((b - a) / n)) for a, b in zip(lo, hi))
    f = scenes.config("C3", 64, 36)
    m = renderer.mesh(f, lo, cell, n, normal=True)
    lift = float(f32(math.sqrt(sum(c * c for c in cell))))
    want = renderer.bake(f, m, cell, lift=lift, materials=scenes.palette(8))
    torch.cuda.synchronize()
    v, t, nrm, col = meshio.read_ply(ply)
    assert same(v, m.verts.cpu().numpy()) and np.array_equal(t, m.tris.cpu().numpy())
    assert same(nrm, m.normal.cpu().numpy())
    assert col is not None and col.shape == (v.shape[0], 3)
    assert np.array_equal(col, meshio.colors_u8(want.cpu().numpy()[:, :3]))
    assert len(np.unique(col, axis=0)) > 50
