"""GPU tests of sdf_mesh_emit_sharp (include/sdf_abi.h "Sharp meshes") against
tests/mesh_sharp_ref.py, the NumPy reference over the CPU oracle.  The reference
takes the crossings' normals as an array: they come from this GPU's
``Renderer.sample_grad`` at the reference's own refined edge points -- the
gradient kernel has its own tests (test_gpu_grad.py) and is not under test here.

Every output buffer is fenced (gpu_support.out_buf: 64 guard rows behind it,
which must survive).  A case's reference is computed once."""
import ctypes as C

import numpy as np
import pytest

import fast_paths as FP
import mesh_ref as M
import mesh_sharp_ref as S
import query_ref as Q
from cases import query_frame
from gpu_support import bitwise_eq, dev, mesh_count, mesh_mismatches, ndiff, out_buf, ptr, raw_mesh
from gpu_support import sdf_main, stream_of, taken
from sdf3d_amd import abi, meshio, renderer as R

pytestmark = pytest.mark.gpu

EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
CENTRE, HALF = S.BOX_CENTRE, S.BOX_HALF
CASES, frame_of = S.CASES, S.frame_of
JIT = ("C4-carved",)     # the run-time specialised seed whose compilations are counted
# Fast precision against the exact reference, sharp (4, 16), C4's fixed variant
# on C4_GRID: the largest |vertex - reference| / cell over the components,
# measured on an MI355X (profiles/mesh_sharp_C4.json fast_deviation).  Every
# fast path is held to 4 x that, the margin fast_paths.MESH_BOUND_V has.
SHARP_MEASURED_V = 1.205e-5
SHARP_BOUND_V = 4 * SHARP_MEASURED_V
_ref, _seen = {}, set()


def emit_sharp(rd, f, g, sharp, ws, nbytes, cap_v, cap_t, normal=True, prim=True):
    """sdf_mesh_emit_sharp into fenced buffers of exactly the capacities given;
    `sharp`: None (a NULL pointer) or (refine, iterations)."""
    torch = rd.torch
    bv = out_buf(rd, cap_v, 3, torch.float32)
    bt = out_buf(rd, cap_t, 3, torch.int32)
    bn = out_buf(rd, cap_v, 3, torch.float32, normal)
    bp = out_buf(rd, cap_v, 1, torch.int32, prim)
    out = abi.sdf_mesh_out(ptr(bv), cap_v, ptr(bt), cap_t, ptr(bn), ptr(bp))
    sp = None if sharp is None else abi.sdf_mesh_sharp(*sharp, 0, 0)
    rc = rd.lib.sdf_mesh_emit_sharp(C.byref(f.scene), C.byref(f.params), C.byref(g), sp, ptr(ws),
                                    nbytes, C.byref(out), stream_of(rd))
    abi.check(rc, "sdf_mesh_emit_sharp")
    torch.cuda.synchronize()
    return {"verts": taken(rd, bv), "tris": taken(rd, bt), "normal": taken(rd, bn),
            "prim": taken(rd, bp)}


def sharp_mesh(rd, case, sharp, prec=EXACT, dense=False):
    """(mesh, run-time compilations of the emit) of `case` through the ABI."""
    scene, spec = CASES[case]
    f, g = frame_of(scene, prec), R.grid(*spec, dense=dense)
    ws, nbytes, cn = mesh_count(rd, f, g)
    n0 = rd.lib.sdf_jit_count()
    got = emit_sharp(rd, f, g, sharp, ws, nbytes, cn[0], cn[1])
    got["counts"] = cn
    return got, rd.lib.sdf_jit_count() - n0


def reference(rd, case, sharp):
    """mesh_sharp_ref of `case` in exact precision, with sdf_sample's normals and
    the owner fold at its vertices; once per (case, sharp)."""
    if (case, sharp) not in _ref:
        scene, spec = CASES[case]
        f = frame_of(scene)
        E = S.edges(f, *spec, 0.0, sharp[0])
        grads = rd.sample_grad(f, dev(rd, E["points"]), grad_prims=False).grad_points
        rd.torch.cuda.synchronize()
        r = S.mesh(E, grads.cpu().numpy(), sharp[1])
        r["normal"] = Q.normals(f, r["verts"])
        r["prim"] = Q.owner(f, r["verts"])[0]
        r["crossings"] = len(E["points"])
        r["plain_verts"] = E["plain"]["verts"]
        _ref[(case, sharp)] = r
    return _ref[(case, sharp)]


def first_compile(case, prec):
    """Run-time compilations the first sharp emit of (case, precision) makes in
    this process: one on the run-time specialised seed, none on a built-in or
    generic path, then none; at most one on the box scenes, which no test counts."""
    scene = CASES[case][0]
    key = ("mesh", "sharp", scene, prec)
    first = key not in _seen
    _seen.add(key)
    if scene.startswith("BOX"):
        return (0, 1) if first and FP.jit_on() else (0,)
    return (1,) if scene in JIT and first and FP.jit_on() else (0,)


# 1. identity ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["C4", "BOX"])
def test_plain_sharp_is_sdf_mesh_emit(renderer, case):
    """sharp NULL and (0, 0): sdf_mesh_emit's verts, tris, normal and prim bit for
    bit.  (4, 0): its tris; the verts are the reference's, whose mass point moved
    only through the refined tau."""
    scene, spec = CASES[case]
    plain = raw_mesh(renderer, frame_of(scene), spec)
    for sharp in (None, (0, 0)):
        got, _ = sharp_mesh(renderer, case, sharp)
        assert got["counts"] == plain["counts"]
        for k in ("verts", "tris", "normal", "prim"):
            assert np.all(bitwise_eq(got[k], plain[k])), (sharp, k)
    want = first_compile(case, EXACT)
    got, jit = sharp_mesh(renderer, case, (4, 0))
    ref = reference(renderer, case, (4, 0))
    assert jit in want
    assert np.array_equal(got["tris"], plain["tris"])
    assert mesh_mismatches(got, ref) == {"verts": 0, "tris": 0, "normal": 0, "prim": 0}
    moved = ndiff(got["verts"], plain["verts"])
    print(f"{case}: {moved} of {got['verts'].size} vertex words moved by the refinement alone")
    assert 0 < moved
    lim = np.asarray(spec[1], dtype=np.float64)
    assert np.nanmax(np.abs(got["verts"].astype(np.float64) - plain["verts"]) / lim) < 1.0


# 2. exact precision -----------------------------------------------------------------
@pytest.mark.parametrize("sharp", [(4, 16), (1, 3)])
@pytest.mark.parametrize("case", ["BOX", "BOX-BALL", "C4", "C4-generic", "C4-unculled", "C4-carved"])
def test_exact_sharp_mesh_equals_the_reference(renderer, case, sharp):
    """verts (bit patterns, NaN equal to NaN), tris, normal and prim equal the
    reference; a run-time specialised scene compiles one more kernel on its
    first sharp emit and none after; SDF_MESH_DENSE changes no bit."""
    want = first_compile(case, EXACT)
    got, jit = sharp_mesh(renderer, case, sharp)
    again, jit_again = sharp_mesh(renderer, case, sharp, dense=True)
    ref = reference(renderer, case, sharp)
    bad = mesh_mismatches(got, ref) if got["counts"][:2] == ref["counts"] else None
    print(f"{case} {sharp}: counts {got['counts']} reference {ref['counts']} crossings "
          f"{ref['crossings']} clamped {ref['clamped']} NaN components "
          f"{int(np.isnan(ref['verts']).sum())} mismatches {bad} compiled {jit}, {jit_again}")
    assert got["counts"][:2] == ref["counts"]
    assert bad == {"verts": 0, "tris": 0, "normal": 0, "prim": 0}
    assert jit in want and jit_again == 0
    assert again["counts"][:2] == got["counts"][:2] and again["counts"][2] == again["counts"][3]
    for k in ("verts", "tris", "normal", "prim"):
        assert np.all(bitwise_eq(got[k], again[k])), k
    if case == "BOX":
        assert got["counts"][3] == 27
    # the fit did something: some vertex is not the plain mesh's
    assert ndiff(got["verts"], ref["plain_verts"]) > 0


# 3. geometry ------------------------------------------------------------------------------
def box_distance(P):
    """|f| of the box in float64, from the formula."""
    q = np.abs(np.asarray(P, dtype=np.float64) - CENTRE) - HALF
    return np.abs(np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0))


def corner_distance(P):
    """The distance from each of the box's 8 corners to the vertex nearest it."""
    sg = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    corners = CENTRE + sg * HALF
    d = np.linalg.norm(np.asarray(P, dtype=np.float64)[None] - corners[:, None], axis=2)
    return d.min(axis=1)


def test_sharp_vertices_lie_on_the_box(renderer):
    """The box on 20^3 cubic cells of 0.05, sharp (4, 16), over all 726 vertices:
    max |f(vertex)| <= 0.1 cell and the vertex nearest each of the 8 corners
    within 0.2 cell of it, where the plain mesh has >= 0.4 cell and >= 0.8 cell
    (f and the distances in float64 NumPy from the box formula).  The bounds are
    the issue's: about 4 x and 3 x a float64 prototype's 0.025 and 0.06.

    mesh_sharp_ref on this grid on the CPU, with float64 autograd gradients of
    the box rounded to fp32 (tests/grad_ref.py), before any GPU run: 0.02524
    cell and 0.05874 cell, no vertex clamped, against the plain mesh's 0.52000
    and 0.98821; signed volume 0.153922 (sharp) and 0.149249 (plain) of the
    box's 0.154008.  The fp32 reference stays within the bounds, so they stand
    as stated."""
    scene, spec = CASES["BOX-cubic"]
    cell = 0.05
    first_compile("BOX-cubic", EXACT)
    got, _ = sharp_mesh(renderer, "BOX-cubic", (4, 16))
    plain = raw_mesh(renderer, frame_of(scene), spec)
    ref = reference(renderer, "BOX-cubic", (4, 16))
    assert got["counts"][:2] == (726, 1448) and np.array_equal(got["tris"], plain["tris"])
    assert mesh_mismatches(got, ref) == {"verts": 0, "tris": 0, "normal": 0, "prim": 0}
    f_sharp, f_plain = box_distance(got["verts"]).max() / cell, box_distance(plain["verts"]).max() / cell
    c_sharp, c_plain = corner_distance(got["verts"]).max() / cell, corner_distance(plain["verts"]).max() / cell
    true = 8.0 * HALF.prod()
    v_sharp = abs(M.signed_volume(got["verts"], got["tris"]) - true)
    v_plain = abs(M.signed_volume(plain["verts"], plain["tris"]) - true)
    print(f"max |f| / cell: sharp {f_sharp:.5f} plain {f_plain:.5f}; corner distance / cell: sharp "
          f"{c_sharp:.5f} plain {c_plain:.5f}; volume error: sharp {v_sharp:.3e} plain {v_plain:.3e}; "
          f"clamped {ref['clamped']}")
    assert f_sharp <= 0.1 and c_sharp <= 0.2
    assert f_plain >= 0.4 and c_plain >= 0.8
    assert v_sharp < v_plain
    # every vertex inside its own cell, and the mesh still closed
    lo = np.asarray(spec[0], dtype=np.float64) + ref["cells"] * cell
    assert np.all(got["verts"] >= lo - 1e-6) and np.all(got["verts"] <= lo + cell + 1e-6)
    assert set(M.edge_uses(got["tris"])) == {2}


# 4. capacities --------------------------------------------------------------------------
def test_capacity_guards_every_store(renderer):
    """max_verts = nv - 3 and max_tris = nt - 5: exactly that prefix is written and
    nothing beyond it (the fence behind every buffer)."""
    first_compile("C4", EXACT)
    full, _ = sharp_mesh(renderer, "C4", (4, 16))
    scene, spec = CASES["C4"]
    f, g = frame_of(scene), R.grid(*spec)
    ws, nbytes, cn = mesh_count(renderer, f, g)
    nv, nt = cn[0] - 3, cn[1] - 5
    got = emit_sharp(renderer, f, g, (4, 16), ws, nbytes, nv, nt)
    assert np.all(bitwise_eq(got["verts"], full["verts"][:nv])) and np.all(got["tris"] == full["tris"][:nt])
    assert np.all(bitwise_eq(got["normal"], full["normal"][:nv])) and np.all(got["prim"] == full["prim"][:nv])
    one = emit_sharp(renderer, f, g, (4, 16), ws, nbytes, nv, 0, normal=False, prim=False)
    assert np.all(bitwise_eq(one["verts"], full["verts"][:nv])) and len(one["tris"]) == 0


# 5. fast precision ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["BOX-cubic", "C4", "C4-generic", "C4-carved"])
def test_fast_sharp_mesh_within_the_measured_bound(renderer, case):
    """Grids whose reference lattice has min |w| >= 1e-4, so no sign can flip:
    counts and triangles equal the reference, two calls give the same bits, some
    vertex word differs from the exact mesh (the fast unit ran), and the
    vertices stay within 4 x the deviation measured on C4's fixed variant."""
    sharp = (4, 16)
    ref = reference(renderer, case, sharp)
    assert ref["min_abs_w"] >= 1e-4
    if CASES[case][0] in FP.JIT:
        FP.first_use(("mesh", "count", CASES[case][0]))    # test_gpu_mesh.py's ledger of that kernel
    want = first_compile(case, FAST)
    got, jit = sharp_mesh(renderer, case, sharp, FAST)
    again, jit_again = sharp_mesh(renderer, case, sharp, FAST)
    assert jit in want and jit_again == 0
    assert got["counts"][:2] == ref["counts"] and np.array_equal(got["tris"], ref["tris"])
    for k in ("verts", "tris", "normal", "prim"):
        assert np.all(bitwise_eq(got[k], again[k])), k
    cell = np.asarray(CASES[case][1][1], dtype=np.float64)
    dv = float((np.abs(got["verts"].astype(np.float64) - ref["verts"]) / cell).max())
    differ = ndiff(got["verts"], ref["verts"])
    print(f"{case}: fast sharp vertex deviation / cell {dv:.3e} (bound {SHARP_BOUND_V:.3e}); words "
          f"differing from the exact mesh {differ}")
    assert dv <= SHARP_BOUND_V
    assert differ > 0, "the exact kernel's bits: the fast unit did not run"


# 6. the wrappers ------------------------------------------------------------------------------
def test_renderer_mesh_sharp_is_the_abi_calls(renderer):
    first_compile("C4", EXACT)
    full, _ = sharp_mesh(renderer, "C4", (4, 16))
    scene, (origin, cell, n) = CASES["C4"]
    m = renderer.mesh(frame_of(scene), origin, cell, n, normal=True, prim=True, sharp=True)
    renderer.torch.cuda.synchronize()
    assert m.counts == full["counts"]
    for k in ("verts", "tris", "normal", "prim"):
        assert np.all(bitwise_eq(getattr(m, k).cpu().numpy(), full[k])), k
    m2 = renderer.mesh(frame_of(scene), origin, cell, n, sharp=(4, 16))
    assert m2.normal is None and np.all(bitwise_eq(m2.verts.cpu().numpy(), full["verts"]))
    plain = renderer.mesh(frame_of(scene), origin, cell, n)
    m0 = renderer.mesh(frame_of(scene), origin, cell, n, sharp=(0, 0))
    assert np.all(bitwise_eq(m0.verts.cpu().numpy(), plain.verts.cpu().numpy()))
    assert ndiff(plain.verts.cpu().numpy(), full["verts"]) > 0


def test_cpp_host_program_mesh_sharp(renderer, tmp_path):
    """sdf_main --mesh FILE.obj --grid ... --mesh-sharp writes the arrays
    Renderer.mesh(sharp=True) gives for its csg8 scene (C3's) on that grid, and
    --mesh-sharp 1,3 those of sharp=(1, 3)."""
    f = query_frame("C3")
    for words, sharp in ((("--mesh-sharp",), True), (("--mesh-sharp", "1,3"), (1, 3))):
        obj = tmp_path / "m.obj"
        r = sdf_main("--mesh", obj, "--grid", "-1.25,-0.125,-1,1.25,1.125,1,20", *words, "64", "36",
                     "1", tmp_path / "f.ppm", "csg8")
        assert r.returncode == 0, r.stderr
        m = renderer.mesh(f, (-1.25, -0.125, -1.0), (0.125, 0.0625, 0.1), 20, normal=True, sharp=sharp)
        renderer.torch.cuda.synchronize()
        v, t, n = meshio.read_obj(obj)
        assert np.all(bitwise_eq(v, m.verts.cpu().numpy())) and np.all(t == m.tris.cpu().numpy())
        assert np.all(bitwise_eq(n, m.normal.cpu().numpy()))
    plain = renderer.mesh(f, (-1.25, -0.125, -1.0), (0.125, 0.0625, 0.1), 20)
    assert ndiff(plain.verts.cpu().numpy(), v) > 0
