"""Reference of the mesh entry points (include/sdf_abi.h "Meshes":
sdf_mesh_count, sdf_mesh_emit), in NumPy over the CPU oracle's point probe
(oracle.scene_sdf, and query_ref's normals and owner fold at the vertices).
TEST INFRASTRUCTURE ONLY.

Every value is fp32, every operation rounded once, nothing fused: NumPy's
float32 element-wise arithmetic is the exact precision's.  Arrays over the
lattice and over the cells are indexed [i2, i1, i0].

  lattice   p.c = origin[c] + (float)i cell[c];  w = f(p) - iso;  inside = w < 0
  vertex    the mean of the crossing edges' local points, edges in increasing
            e = 4a + s + 2t, then origin-corner + g cell
  order     (brick, local) over bricks of 8 x 8 x 8 cells
  quads     edge 4a of an active cell with i_u >= 1 and i_v >= 1
"""
import numpy as np

import query_ref as Q

f32 = np.float32


def axes(origin, cell, n):
    """The lattice coordinates per axis: RN(origin + RN((float)i cell))."""
    return [(f32(origin[c]) + np.arange(n[c] + 1).astype(f32) * f32(cell[c])).astype(f32)
            for c in range(3)]


def lattice(frame, origin, cell, n, iso=0.0):
    """(ax, w): w[i2, i1, i0] = RN(f(p) - iso) with f the oracle's scene SDF."""
    ax = axes(origin, cell, n)
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1).astype(f32)
    with np.errstate(all="ignore"):
        w = (Q.scene_sdf(frame, P) - f32(iso)).astype(f32)
    return ax, w.reshape(n[2] + 1, n[1] + 1, n[0] + 1)


def _corner(a, off, n):
    """The lattice array `a` at the cells' corner `off` = (d0, d1, d2)."""
    return a[off[2]:off[2] + n[2], off[1]:off[1] + n[1], off[0]:off[0] + n[0]]


def extract(ax, w, cell, n):
    """The mesh of a lattice: dict of verts (nv, 3) float32, tris (nt, 3) int32,
    cells (nv, 3) the vertices' cell indices (i0, i1, i2), bricks (active
    bricks, all bricks)."""
    n = tuple(int(x) for x in n)
    inside = w < 0                                   # a NaN or a zero is outside
    cnt = np.zeros((n[2], n[1], n[0]), dtype=np.int32)
    for k in range(8):
        cnt += _corner(inside, (k & 1, (k >> 1) & 1, k >> 2), n)
    active = (cnt > 0) & (cnt < 8)
    S = [np.zeros(active.shape, dtype=f32) for _ in range(3)]
    m = np.zeros(active.shape, dtype=np.int32)
    with np.errstate(all="ignore"):
        for a in range(3):
            u, v = (a + 1) % 3, (a + 2) % 3
            for t in (0, 1):
                for s in (0, 1):                     # e = 4a + s + 2t, increasing
                    A = [0, 0, 0]
                    A[u], A[v] = s, t
                    B = list(A)
                    B[a] = 1
                    wa, wb = _corner(w, A, n), _corner(w, B, n)
                    cross = (wa < 0) != (wb < 0)
                    tau = (wa / (wa - wb).astype(f32)).astype(f32)
                    S[a] = np.where(cross, (S[a] + tau).astype(f32), S[a])
                    S[u] = np.where(cross, (S[u] + f32(s)).astype(f32), S[u])
                    S[v] = np.where(cross, (S[v] + f32(t)).astype(f32), S[v])
                    m += cross
        I = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
        idx = [I[2], I[1], I[0]]                     # i0, i1, i2 per cell
        pos = []
        for c in range(3):
            g = (S[c] / m.astype(f32)).astype(f32)
            pos.append((ax[c][idx[c]] + (g * f32(cell[c])).astype(f32)).astype(f32))
    nb = [(n[c] + 7) // 8 for c in range(3)]
    brick = ((idx[2] // 8) * nb[1] + idx[1] // 8) * nb[0] + idx[0] // 8
    local = ((idx[2] % 8) * 8 + idx[1] % 8) * 8 + idx[0] % 8
    key = brick.astype(np.int64) * 512 + local
    sel = np.nonzero(active.ravel())[0]
    sel = sel[np.argsort(key.ravel()[sel], kind="stable")]
    vid = np.full(active.size, -1, dtype=np.int64)
    vid[sel] = np.arange(len(sel))
    vid = vid.reshape(active.shape)
    verts = np.stack([p.ravel()[sel] for p in pos], axis=1).astype(f32).reshape(-1, 3)
    cells = np.stack([idx[c].ravel()[sel] for c in range(3)], axis=1)
    # quads: per active cell in order, a = 0, 1, 2
    in0 = _corner(inside, (0, 0, 0), n)
    quads, order = [], []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        B = [0, 0, 0]
        B[a] = 1
        emit = active & (in0 != _corner(inside, B, n)) & (idx[u] >= 1) & (idx[v] >= 1)
        e = np.nonzero(emit.ravel())[0]
        c = [idx[k].ravel()[e] for k in range(3)]

        def at(du, dv):
            j = [x.copy() for x in c]
            j[u] -= du
            j[v] -= dv
            return vid[j[2], j[1], j[0]]
        q = np.stack([at(1, 1), at(0, 1), at(0, 0), at(1, 0)], axis=1)     # K0 K1 K2 K3
        assert q.size == 0 or q.min() >= 0
        rev = ~in0.ravel()[e]
        q[rev] = q[rev][:, ::-1]
        quads.append(q)
        order.append(vid.ravel()[e] * 3 + a)
    q = np.concatenate(quads)
    q = q[np.argsort(np.concatenate(order), kind="stable")]
    tris = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    active_bricks = len(np.unique(brick.ravel()[sel]))
    return {"verts": verts, "tris": tris, "cells": cells, "bricks": (active_bricks, int(np.prod(nb)))}


def mesh(frame, origin, cell, n, iso=0.0, normal=True, prim=True):
    """The reference of Renderer.mesh in exact precision: dict of verts, tris,
    normal, prim, counts (nv, nt), bricks, and min_abs_w (the lattice value
    closest to a change of sign)."""
    cell = (cell,) * 3 if isinstance(cell, (int, float)) else tuple(cell)
    n = (n,) * 3 if isinstance(n, int) else tuple(n)
    ax, w = lattice(frame, origin, cell, n, iso)
    r = extract(ax, w, cell, n)
    r["counts"] = (len(r["verts"]), len(r["tris"]))
    with np.errstate(all="ignore"):
        r["min_abs_w"] = float(np.nanmin(np.abs(w)))
    r["zeros"] = int((w == 0).sum())
    r["normal"] = Q.normals(frame, r["verts"]) if normal else None
    r["prim"] = Q.owner(frame, r["verts"])[0] if prim else None
    return r


def edge_uses(tris):
    """How often each undirected edge is used: the sorted counts' histogram
    {uses: edges}."""
    t = np.asarray(tris, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = np.sort(e, axis=1)
    _, c = np.unique(e, axis=0, return_counts=True)
    u, k = np.unique(c, return_counts=True)
    return {int(a): int(b) for a, b in zip(u, k)}


def signed_volume(verts, tris):
    P = np.asarray(verts, dtype=np.float64)
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


def fast_deviation(ref, got, cell):
    """A fast-precision mesh (`got`: counts, verts, tris, normal, prim as NumPy)
    against the reference `ref` of mesh(): whether counts and triangles are the
    reference's, and then the largest |vertex - reference| / cell over the
    components and the largest normal-component difference."""
    cell = np.asarray((cell,) * 3 if isinstance(cell, (int, float)) else cell, dtype=np.float64)
    ok = tuple(got["counts"][:2]) == tuple(ref["counts"]) and np.array_equal(got["tris"], ref["tris"])
    dv = dn = float("inf")
    wrong = -1
    if ok:
        dv = float((np.abs(got["verts"].astype(np.float64) - ref["verts"]) / cell).max())
        dn = float(np.abs(got["normal"].astype(np.float64) - ref["normal"]).max())
        wrong = int((got["prim"] != ref["prim"]).sum())
    return {"min_abs_w": ref["min_abs_w"], "same_connectivity": bool(ok), "vertex_over_cell": dv,
            "normal": dn, "prim_wrong": wrong}
