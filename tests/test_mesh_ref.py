"""The mesh reference itself (tests/mesh_ref.py), sanity-checked on the CPU on
C1, the sphere of radius 0.2: a closed 2-manifold that is oriented outwards,
with the vertex and triangle counts of the definition's prototype, and a grid
with a lattice value of exactly 0 ("a zero is outside")."""
import numpy as np

import mesh_ref as M
from sdf3d_amd import scenes

OFF = ((-0.31, 0.13, -0.29), (0.05, 0.06, 0.055), (12, 10, 11))
ZERO = ((-0.3, 0.1, -0.3), 0.05, 12)


def test_sphere_is_closed_manifold_and_oriented():
    f = scenes.config("C1", 64, 64)
    r = M.mesh(f, *OFF)
    vol = M.signed_volume(r["verts"], r["tris"])
    print(f"C1 offset grid: counts {r['counts']} edge uses {M.edge_uses(r['tris'])} volume {vol:.5f} "
          f"min |w| {r['min_abs_w']:.3e}")
    assert r["counts"] == (242, 480)
    assert M.edge_uses(r["tris"]) == {2: 720}          # every undirected edge exactly twice
    assert vol > 0 and abs(vol - 0.0307) < 5e-4        # the prototype's; the sphere's own is 0.0335
    assert np.isfinite(r["verts"]).all() and r["tris"].min() == 0
    assert r["tris"].max() == len(r["verts"]) - 1
    # normals point out of the inside: along the vertex's direction from the centre
    c = np.array([0.0, 0.4, 0.0])
    d = r["verts"].astype(np.float64) - c
    assert (np.einsum("ij,ij->i", d, r["normal"].astype(np.float64)) > 0).all()
    assert (r["prim"] == 0).all()


def test_a_zero_is_outside():
    f = scenes.config("C1", 64, 64)
    r = M.mesh(f, *ZERO, normal=False, prim=False)
    print(f"C1 grid with a zero: counts {r['counts']} zeros {r['zeros']}")
    assert r["zeros"] == 1
    assert r["counts"] == (280, 556)
    assert set(M.edge_uses(r["tris"])) == {2}


def test_offset_shell_is_larger():
    f = scenes.config("C1", 64, 64)
    r0 = M.mesh(f, *OFF, normal=False, prim=False)
    r1 = M.mesh(f, *OFF, iso=0.05, normal=False, prim=False)
    assert M.signed_volume(r1["verts"], r1["tris"]) > M.signed_volume(r0["verts"], r0["tris"])
    assert set(M.edge_uses(r1["tris"])) == {2}
