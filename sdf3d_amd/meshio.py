"""Wavefront OBJ and binary PLY files for the meshes of ``Renderer.mesh``
(sdf_mesh_emit) and the vertex colours of ``Renderer.bake`` (sdf_shade_points).

``write_obj`` takes host arrays (NumPy, or anything ``numpy.asarray`` accepts;
move device tensors to the host first): one ``v`` line per vertex, one ``vn``
line per vertex when normals are given, one ``f`` line per triangle with
1-based indices (``f a//a b//b c//c`` with normals).  Floats are written with
nine significant digits, which round-trips fp32 exactly; NaN and infinities
are written as Python spells them and read back the same.  With `colors` a
``v`` line carries the vertex colour behind the position (``v x y z r g b``,
the extension most viewers read), as floats.

``write_ply`` / ``read_ply`` are binary little-endian PLY: float x y z per
vertex, then float nx ny nz when normals are given, then uchar red green blue
when colours are given, and one ``uchar 3, int a b c`` list per triangle.  A
colour component becomes a byte by the RGBA8 rule of include/sdf_abi.h:
``u8 = trunc(min(max(c, 0), 1) * 255 + 0.5)`` in fp32, NaN -> 0 (``colors_u8``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np


def _mesh_arrays(verts, tris, normals, colors):
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    if n is not None and len(n) != len(v):
        raise ValueError("one normal per vertex")
    c = None
    if colors is not None:
        c = np.asarray(colors)
        if c.ndim != 2 or c.shape[0] != len(v) or c.shape[1] not in (3, 4):
            raise ValueError("one colour (r, g, b[, a]) per vertex")
        c = c[:, :3]
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle refers to a vertex that is not there")
    return v, t, n, c


def colors_u8(colors) -> np.ndarray:
    """Float colours as bytes by the RGBA8 rule of include/sdf_abi.h: u8 =
    trunc(min(max(c, 0), 1) * 255 + 0.5) in fp32, a NaN gives 0.  Arrays of
    bytes pass through."""
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    c = c.astype(np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(c), np.float32(0.0), np.minimum(np.maximum(c, np.float32(0.0)),
                                                              np.float32(1.0))).astype(np.float32)
        x = (x * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    return np.trunc(x.astype(np.float32)).astype(np.uint8)


def write_obj(path, verts, tris, normals=None, colors=None) -> None:
    v, t, n, c = _mesh_arrays(verts, tris, normals, colors)
    lines = [f"# {len(v)} vertices, {len(t)} triangles"]
    if c is None:
        lines += ["v %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in v]
    else:
        c = c.astype(np.float32)
        lines += ["v %.9g %.9g %.9g %.9g %.9g %.9g" % tuple(float(x) for x in (*p, *q))
                  for p, q in zip(v, c)]
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


def write_ply(path, verts, tris, normals=None, colors=None) -> None:
    """Binary little-endian PLY (see the module's text).  `colors`: (nv, 3) or
    (nv, 4) floats, converted by ``colors_u8``, or bytes; alpha is not written."""
    v, t, n, c = _mesh_arrays(verts, tris, normals, colors)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
            "property float x", "property float y", "property float z"]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros(len(v), dtype=np.dtype(fields))
    for i, k in enumerate("xyz"):
        rec[k] = v[:, i]
        if n is not None:
            rec["n" + k] = n[:, i]
    if c is not None:
        u = colors_u8(c)
        for i, k in enumerate(("red", "green", "blue")):
            rec[k] = u[:, i]
    faces = np.zeros(len(t), dtype=np.dtype([("k", "u1"), ("i", "<i4", (3,))]))
    faces["k"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """(verts (nv, 3) float32, tris (nt, 3) int32, normals (nv, 3) float32 or
    None, colors (nv, 3) uint8 or None) of a PLY file as ``write_ply`` writes
    them."""
    data = Path(path).read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY file")
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    nv = nt = 0
    fields, element = [], None
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nt = int(w[2])
            else:
                raise ValueError(f"unknown element {element!r}")
        elif w[0] == "property" and element == "vertex":
            fields.append((w[2], types[w[1]]))
        elif w[0] == "property" and w[1:4] != ["list", "uchar", "int"]:
            raise ValueError(f"unknown face property: {line!r}")
    vt = np.dtype(fields)
    ft = np.dtype([("k", "u1"), ("i", "<i4", (3,))])
    if len(data) != end + nv * vt.itemsize + nt * ft.itemsize:
        raise ValueError("the file's length does not match its header")
    rec = np.frombuffer(data, dtype=vt, count=nv, offset=end)
    faces = np.frombuffer(data, dtype=ft, count=nt, offset=end + nv * vt.itemsize)
    if nt and (faces["k"] != 3).any():
        raise ValueError("not a triangle mesh")
    names = set(vt.names)
    verts = np.stack([rec[k] for k in "xyz"], axis=-1).astype(np.float32).reshape(-1, 3)
    normals = (np.stack([rec["n" + k] for k in "xyz"], axis=-1).astype(np.float32).reshape(-1, 3)
               if {"nx", "ny", "nz"} <= names else None)
    colors = (np.stack([rec[k] for k in ("red", "green", "blue")], axis=-1).reshape(-1, 3)
              if {"red", "green", "blue"} <= names else None)
    return verts, faces["i"].astype(np.int32).reshape(-1, 3), normals, colors
