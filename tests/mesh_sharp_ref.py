"""Reference of sdf_mesh_emit_sharp (include/sdf_abi.h "Sharp meshes"), in NumPy
fp32 over mesh_ref's lattice and extraction.  TEST INFRASTRUCTURE ONLY.

Two halves, because the crossings' normals are not computed here:

  edges(frame, origin, cell, n, iso, refine)
      the lattice, the plain mesh (numbering, triangles, cells) and every
      crossing lattice edge refined `refine` times with the CPU oracle's scene
      value (query_ref.scene_sdf); `points` are the final edge points, in a
      fixed order, at which the caller evaluates the scene's gradient;
  mesh(E, grads, iterations)
      the fit and the vertices from those gradients ((len(points), 3) fp32).

Every value is fp32 and every operation is rounded once, as in mesh_ref.py.
Arrays over the lattice, its edges and the cells are indexed [i2, i1, i0]; the
array of the edges along a has one entry less along a than the lattice.

Also the scenes and grids of the sharp-mesh tests and of tools/mesh_sharp_probe.py
(CASES, frame_of): a box off the lattice, the box minus a sphere at one corner,
and C4 on its dispatch paths.
"""
import numpy as np

import mesh_ref as M
import query_ref as Q
from cases import C4_GRID, _three, query_frame
from sdf3d_amd import abi

f32 = np.float32

BOX_CENTRE, BOX_HALF = np.array([0.013, 0.021, -0.017]), np.array([0.31, 0.23, 0.27])
BOX = (abi.PRIM_BOX, abi.OP_UNION, 0.0, *BOX_CENTRE, *BOX_HALF)
BALL = (abi.PRIM_SPHERE, abi.OP_SUBTRACT, 0.0, *(BOX_CENTRE + BOX_HALF), 0.2)   # at one corner
# partial bricks, 3 x 3 x 3 = 27 of them
BOX_GRID = ((-0.5, -0.5, -0.5), (0.05, 0.055, 0.045), (20, 19, 21))
CUBIC = ((-0.5, -0.5, -0.5), (0.05, 0.05, 0.05), (20, 20, 20))
# case -> (scene, grid); every scene is a primitive list, BOX, BOX-BALL and
# C4-carved run-time specialised under SDF_DISPATCH_AUTO
CASES = {
    "BOX": ("BOX", BOX_GRID), "BOX-BALL": ("BOX-BALL", BOX_GRID), "BOX-cubic": ("BOX", CUBIC),
    "C4": ("C4", C4_GRID), "C4-generic": ("C4-generic", C4_GRID),
    "C4-unculled": ("C4-unculled", C4_GRID), "C4-carved": ("C4-carved", C4_GRID),
}


def frame_of(scene, prec=abi.PRECISION_EXACT):
    """The frame of a scene of CASES in a precision."""
    if scene.startswith("BOX"):
        return _three(prec, (64, 36), [BOX, BALL] if scene == "BOX-BALL" else [BOX])
    return query_frame(scene, prec)


def _edge_ends(w, a):
    """(w_A, w_B) of every lattice edge along axis a."""
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[2 - a], hi[2 - a] = slice(0, -1), slice(1, None)
    return w[tuple(lo)], w[tuple(hi)]


def edges(frame, origin, cell, n, iso=0.0, refine=0):
    cell = (cell,) * 3 if isinstance(cell, (int, float)) else tuple(cell)
    n = (n,) * 3 if isinstance(n, int) else tuple(int(x) for x in n)
    ax, w = M.lattice(frame, origin, cell, n, iso)
    E = {"frame": frame, "ax": ax, "w": w, "cell": cell, "n": n, "plain": M.extract(ax, w, cell, n),
         "cross": [], "tau": [], "where": []}
    with np.errstate(all="ignore"):
        E["min_abs_w"] = float(np.nanmin(np.abs(w)))
    points = []
    for a in range(3):
        wa, wb = _edge_ends(w, a)
        cross = (wa < 0) != (wb < 0)
        sel = np.nonzero(cross)                         # (i2, i1, i0) of each crossing's corner A
        A = np.stack([ax[0][sel[2]], ax[1][sel[1]], ax[2][sel[0]]], axis=1).astype(f32)
        wa, wb = wa[sel].astype(f32), wb[sel].astype(f32)
        ta, tb = np.zeros(len(wa), dtype=f32), np.ones(len(wa), dtype=f32)

        def at(tau):
            P = A.copy()
            P[:, a] = (A[:, a] + (tau * f32(cell[a])).astype(f32)).astype(f32)
            return P
        with np.errstate(all="ignore"):
            tau = (wa / (wa - wb).astype(f32)).astype(f32)
            for _ in range(refine):                     # always all of them
                wm = (Q.scene_sdf(frame, at(tau)) - f32(iso)).astype(f32) if len(tau) else tau
                same = (wm < 0) == (wa < 0)
                ta, wa = np.where(same, tau, ta), np.where(same, wm, wa)
                tb, wb = np.where(same, tb, tau), np.where(same, wb, wm)
                step = ((tb - ta).astype(f32) * (wa / (wa - wb).astype(f32)).astype(f32)).astype(f32)
                tau = (ta + step).astype(f32)
            points.append(at(tau))
        E["cross"].append(cross)
        E["tau"].append(tau)
        E["where"].append(sel)
    E["points"] = np.concatenate(points).astype(f32).reshape(-1, 3)
    return E


def mesh(E, grads, iterations):
    """dict of verts, tris, cells, counts, clamped (vertices a clamp moved), x
    (the fit's offsets, for diagnosis) from the crossings' gradients."""
    cell, n, ax = E["cell"], E["n"], E["ax"]
    grads = np.asarray(grads, dtype=f32).reshape(-1, 3)
    assert len(grads) == len(E["points"])
    tau_at, nrm_at, first = [], [], 0
    for a in range(3):
        k = len(E["tau"][a])
        t = np.full(E["cross"][a].shape, np.nan, dtype=f32)
        g = np.full(E["cross"][a].shape + (3,), np.nan, dtype=f32)
        t[E["where"][a]] = E["tau"][a]
        g[E["where"][a]] = grads[first:first + k]
        first += k
        tau_at.append(t)
        nrm_at.append(g)
    shape = (n[2], n[1], n[0])
    zero = lambda: np.zeros(shape, dtype=f32)
    S, m = [zero() for _ in range(3)], np.zeros(shape, dtype=np.int32)
    per_edge = []                                       # (a, s, t, cross, tau, normal) in increasing e
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for t in (0, 1):
            for s in (0, 1):
                A = [0, 0, 0]
                A[u], A[v] = s, t
                cross = M._corner(E["cross"][a], A, n)
                tau = M._corner(tau_at[a], A, n)
                nrm = nrm_at[a][A[2]:A[2] + n[2], A[1]:A[1] + n[1], A[0]:A[0] + n[0]]
                per_edge.append((a, s, t, cross, tau, nrm))
    with np.errstate(all="ignore"):
        for a, s, t, cross, tau, _ in per_edge:
            u, v = (a + 1) % 3, (a + 2) % 3
            S[a] = np.where(cross, (S[a] + tau).astype(f32), S[a])
            S[u] = np.where(cross, (S[u] + f32(s)).astype(f32), S[u])
            S[v] = np.where(cross, (S[v] + f32(t)).astype(f32), S[v])
            m += cross
        g = [(S[c] / m.astype(f32)).astype(f32) for c in range(3)]
        AA = {ij: zero() for ij in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
        B = [zero() for _ in range(3)]
        for a, s, t, cross, tau, nrm in per_edge:
            u, v = (a + 1) % 3, (a + 2) % 3
            q = [None] * 3
            q[a], q[u], q[v] = tau, np.full(shape, s, dtype=f32), np.full(shape, t, dtype=f32)
            r = [((q[c] - g[c]).astype(f32) * f32(cell[c])).astype(f32) for c in range(3)]
            nn = [nrm[..., c] for c in range(3)]
            b = (((nn[0] * r[0]).astype(f32) + (nn[1] * r[1]).astype(f32)).astype(f32)
                 + (nn[2] * r[2]).astype(f32)).astype(f32)
            for (i, j) in AA:
                AA[(i, j)] = np.where(cross, (AA[(i, j)] + (nn[i] * nn[j]).astype(f32)).astype(f32),
                                      AA[(i, j)])
            for i in range(3):
                B[i] = np.where(cross, (B[i] + (nn[i] * b).astype(f32)).astype(f32), B[i])
        tr = ((AA[(0, 0)] + AA[(1, 1)]).astype(f32) + AA[(2, 2)]).astype(f32)
        alpha = (f32(1) / tr).astype(f32)
        x = [zero() for _ in range(3)]
        sym = lambda i, j: AA[(min(i, j), max(i, j))]
        for _ in range(iterations):
            d = []
            for i in range(3):
                ax_ = (((sym(i, 0) * x[0]).astype(f32) + (sym(i, 1) * x[1]).astype(f32)).astype(f32)
                       + (sym(i, 2) * x[2]).astype(f32)).astype(f32)
                d.append((B[i] - ax_).astype(f32))
            x = [(x[i] + (alpha * d[i]).astype(f32)).astype(f32) for i in range(3)]
        ok = (tr > 0) & np.isfinite(tr) & np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
        x = [np.where(ok, x[i], f32(0)) for i in range(3)]
        cells = E["plain"]["cells"]
        at = (cells[:, 2], cells[:, 1], cells[:, 0])
        verts, clamped = [], np.zeros(len(cells), dtype=bool)
        for c in range(3):
            free = (g[c] + (x[c] / f32(cell[c])).astype(f32)).astype(f32)
            l = np.where(free < 0, f32(0), free)        # max(x, 0) = x < 0 ? 0 : x
            l = np.where(f32(1) < l, f32(1), l)          # min(x, 1) = 1 < x ? 1 : x
            clamped |= (l != free)[at] & ~np.isnan(free[at])
            verts.append((ax[c][cells[:, c]] + (l * f32(cell[c])).astype(f32)[at]).astype(f32))
    verts = np.stack(verts, axis=1).astype(f32).reshape(-1, 3)
    return {"verts": verts, "tris": E["plain"]["tris"], "cells": cells,
            "counts": (len(verts), len(E["plain"]["tris"])), "bricks": E["plain"]["bricks"],
            "clamped": int(clamped.sum()), "min_abs_w": E["min_abs_w"],
            "x": np.stack([x[c][at] for c in range(3)], axis=1)}
