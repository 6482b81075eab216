"""Wavefront OBJ files for the meshes of ``Renderer.mesh`` (sdf_mesh_emit).

``write_obj`` takes host arrays (NumPy, or anything ``numpy.asarray`` accepts;
move device tensors to the host first): one ``v`` line per vertex, one ``vn``
line per vertex when normals are given, one ``f`` line per triangle with
1-based indices (``f a//a b//b c//c`` with normals).  Floats are written with
nine significant digits, which round-trips fp32 exactly; NaN and infinities
are written as Python spells them and read back the same.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np


def write_obj(path, verts, tris, normals=None) -> None:
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    if n is not None and len(n) != len(v):
        raise ValueError("one normal per vertex")
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle refers to a vertex that is not there")
    lines = [f"# {len(v)} vertices, {len(t)} triangles"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in v]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in n]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in (t + 1).tolist()]
    else:
        lines += ["f %d %d %d" % (a, b, c) for a, b, c in (t + 1).tolist()]
    Path(path).write_text("\n".join(lines) + "\n")


def read_obj(path):
    """(verts (nv, 3) float32, tris (nt, 3) int32, normals (nv, 3) float32 or
    None) of an OBJ file of triangles as ``write_obj`` writes them."""
    v, n, t = [], [], []
    for line in Path(path).read_text().splitlines():
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:4]])
        elif w[0] == "vn":
            n.append([float(x) for x in w[1:4]])
        elif w[0] == "f":
            if len(w) != 4:
                raise ValueError(f"not a triangle: {line!r}")
            t.append([int(x.split("/")[0]) - 1 for x in w[1:4]])
    verts = np.array(v, dtype=np.float32).reshape(-1, 3)
    tris = np.array(t, dtype=np.int32).reshape(-1, 3)
    normals = np.array(n, dtype=np.float32).reshape(-1, 3) if n else None
    return verts, tris, normals
