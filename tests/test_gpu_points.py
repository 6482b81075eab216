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
Every call writes into the middle of sentinel-filled buffers: the GUARD rows in
front of every output and those behind it must survive."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lights_ref as LR
import materials_ref as MR
import oracle
import points_ref as PR
from sdf3d_amd import abi, meshio, renderer as R, scenes
from test_gpu_materials import both as frame_both
from test_gpu_materials import render as frame_render
from test_gpu_ssaa import FILL

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
A, G, U = abi.DISPATCH_AUTO, abi.DISPATCH_GENERIC, abi.DISPATCH_UNCULLED
CLR = abi.LIGHTS_COLOR
W, H = MR.SHAPE
N = W * H
LIGHTS = LR.rig(8)
OUTS = ("rgba", "ao", "shadow", "material", "steps")
ROOT = Path(__file__).resolve().parent.parent

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


# ---- helpers ---------------------------------------------------------------------------

def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8),
                                                                        b.view(np.uint8))


def ndiff(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
               .sum())


def points_scene(prec, counted=False):
    """capsule, plane, torus (smooth union) -- `counted`: torus, plane, capsule:
    no built-in variant, so SDF_DISPATCH_AUTO compiles its kernel at run time
    (hipRTC); `counted` is used only by the test that counts its compilations."""
    f = scenes.config("C3", W, H, precision=prec, pose=2)
    C.memset(C.addressof(f.scene.prims), 0, C.sizeof(f.scene.prims))
    f.scene.count = 3
    cap = (abi.PRIM_CAPSULE, -0.4, 0.15, 0.1, 0.1, 0.5, -0.1, 0.12)
    tor = (abi.PRIM_TORUS, 0.45, 0.12, 0.0, 0.25, 0.08)
    first, last = (tor, cap) if counted else (cap, tor)
    scenes._prim(f.scene, 0, first[0], abi.OP_UNION, 0.0, *first[1:])
    scenes._prim(f.scene, 1, abi.PRIM_PLANE, abi.OP_UNION, 0.0, 0.0, 1.0, 0.0, 0.0)
    scenes._prim(f.scene, 2, last[0], abi.OP_SMOOTH_UNION, 0.08, *last[1:])
    f.params.dispatch = A
    return f


def the_frame(name, pose, prec=EXACT, dispatch=A):
    if name in ("PJ", "PJC"):
        return points_scene(prec, counted=name == "PJC")
    f = scenes.config(name, W, H, precision=prec, pose=pose)
    f.params.dispatch = dispatch
    return f


def mats_of(f, pal=True):
    if f.scene.kind != abi.SCENE_PRIMITIVES:
        return [f.material]
    return scenes.palette(f.scene.count) if pal else [f.material] * f.scene.count


GUARD = 64   # sentinel rows in front of and behind every output (a wave's worth)


def fenced(torch, device, shape, dtype):
    """A sentinel-filled allocation of GUARD + shape[0] + GUARD rows: the kernel is
    handed rows GUARD .. GUARD + shape[0].  (GUARD rows of any output are a
    multiple of 16 bytes, so `rgba` stays aligned.)"""
    rows = shape[0] + 2 * GUARD
    nbytes = rows * int(np.prod(shape[1:])) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes,), FILL, dtype=torch.uint8, device=device)
    return raw.view(dtype).reshape(rows, *shape[1:])


def untouched(torch, x):
    return bool((x.contiguous().view(-1).view(torch.uint8) == FILL).all())


def shade(rd, f, P, normals=None, eye=None, lift=0.0, lights=None, flags=0, materials=None,
          outs=OUTS):
    """sdf_shade_points into the middle of sentinel-filled buffers whose guard
    rows, in front of every output and behind it, are checked: a
    points_ref.RefShade of NumPy arrays (None for an output not in `outs`; dif is
    not an output)."""
    import torch
    dev = lambda a: torch.from_numpy(np.array(a, dtype=f32).reshape(-1, 3)).to(rd.device)
    pts = dev(P)
    n = pts.shape[0]
    nrm = None if normals is None else dev(normals)
    lights = [f.light] if lights is None else list(lights)
    materials = mats_of(f, False) if materials is None else list(materials)
    nl = len(lights)
    larr = (abi.sdf_light * nl)(*lights)
    marr = (abi.sdf_material * len(materials))(*materials)
    shapes = {"rgba": ((n, 4), torch.float32), "ao": ((n,), torch.float32),
              "shadow": ((n, nl), torch.float32), "material": ((n, 9), torch.float32),
              "steps": ((n, nl), torch.int32)}
    bufs = {k: fenced(torch, rd.device, *shapes[k]) for k in outs}
    mid = {k: b[GUARD:GUARD + n] for k, b in bufs.items()}
    p = abi.sdf_points()
    p.points, p.n, p.lift = pts.data_ptr(), n, float(lift)
    p.normals = nrm.data_ptr() if nrm is not None else None
    if eye is not None:
        p.flags = abi.POINTS_EYE
        for c in range(3):
            p.eye[c] = float(eye[c])
    ps = abi.sdf_point_shade(*[mid[k].data_ptr() if k in mid else None for k in OUTS])
    rc = rd.lib.sdf_shade_points(C.byref(f.scene), larr, nl, int(flags), marr, len(materials),
                                 C.byref(f.params), C.byref(p), C.byref(ps), None)
    torch.cuda.synchronize()
    assert rc == abi.SDF_OK, rc
    for k, b in bufs.items():
        assert untouched(torch, b[:GUARD]), f"{k}: entries in front of the buffer were written"
        assert untouched(torch, b[GUARD + n:]), f"{k}: entries past the end were written"
    got = {k: (mid[k].cpu().numpy() if k in mid else None) for k in OUTS}
    return PR.RefShade(got["rgba"], got["ao"], got["shadow"], got["material"], got["steps"], None)


_HITS = {}


def hit_points(rd, name, pose):
    """(P (851, 3), eye) of the exact frame: P_0 = O_0 + D_0 d formed on the host
    in unfused fp32 from trace_camera's t and camera_rays, as the render forms
    it."""
    if (name, pose) not in _HITS:
        assert (W, H) == (37, 23) and N == 851 == 13 * 64 + 19
        f = the_frame(name, pose)
        t = rd.trace_camera(f, normal=False, prim=False, steps=False).t
        o, d = rd.camera_rays(f)
        rd.torch.cuda.synchronize()
        o, d, t = o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()
        P = PR.hit_points(o, d, t).reshape(N, 3)
        eye = o.reshape(N, 3)[0].copy()
        assert same(o.reshape(N, 3), np.tile(eye, (N, 1)))
        P.setflags(write=False)
        _HITS[(name, pose)] = (P, eye)
    return _HITS[(name, pose)]


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
    want, want_st = frame_both(renderer, f, mats, [f.light], 0)
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

FAST_CASES = [("C4", 0, False), ("C3", 2, True), ("REF", 0, True)]


def fast_deviation(rd, name, pose, pal):
    """The largest absolute deviation of each output of the fast kernel from the
    reference replayed at the kernel's own shadow counts, over all 851 hit
    points under three coloured lights (`material`: where no hard decision of
    the fold is closer than materials_ref.GAP), and how many points that is."""
    f = the_frame(name, pose, FAST)
    mats = mats_of(f, pal)
    P, eye = hit_points(rd, name, pose)
    got = shade(rd, f, P, eye=eye, lights=LIGHTS[:3], flags=CLR, materials=mats)
    ref = PR.shade(the_frame(name, pose), P, eye=eye, lights=LIGHTS[:3], light_flags=CLR,
                   materials=mats, steps=got.steps)
    assert np.array_equal(ref.steps, np.minimum(got.steps, f.params.max_steps))
    dev = {}
    for k in ("rgba", "ao", "shadow"):
        a, b = getattr(got, k).astype(np.float64), getattr(ref, k).astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        dev[k] = float(np.abs(a - b).max())
    gap = np.array([MR.fold_at(f.scene, mats, *map(float, p))[2] for p in P], dtype=f32)
    far = ~(gap < f32(MR.GAP))
    dev["material"] = float(np.abs(got.material[far].astype(np.float64) -
                                   ref.material[far].astype(np.float64)).max())
    return dev, int(far.sum())


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
    exe = ROOT / "sdf3d_amd" / "bin" / "sdf_main"
    assert exe.exists(), "build() must produce sdf3d_amd/bin/sdf_main"
    ply = tmp_path / "m.ply"
    n = BAKE_N
    lo = [float(x) for x in BAKE_ORIGIN]
    hi = [a + BAKE_CELL * n for a in lo]
    r = subprocess.run([str(exe), "--palette", "--mesh", str(ply), "--mesh-colors", "--grid",
                        ",".join(repr(x) for x in (*lo, *hi)) + f",{n}", "64", "36", "1",
                        str(tmp_path / "f.ppm"), "csg8"], capture_output=True, text=True,
                       timeout=120)
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
