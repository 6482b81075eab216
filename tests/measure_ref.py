"""Reference of sdf_measure (include/sdf_abi.h "Measures"), in NumPy over the
CPU oracle's point probe (query_ref.scene_sdf) and owner fold (query_ref.owner).
TEST INFRASTRUCTURE ONLY.

Every sample position is fp32, every operation rounded once, nothing fused:
NumPy's float32 element-wise arithmetic is the exact precision's.  The sums are
Python / NumPy int64 over index arrays: exact.  Arrays over the samples are
indexed [i2, i1, i0].

  sample    p.c = origin[c] + ((float)i + 0.5f) cell[c];  w = f(p) - iso;  inside = w < 0
  row       N, S (3), Q (00 11 22 01 02 12), lo (3), hi (3); empty: 0 .., n, -1
  bricks    8 x 8 x 8 samples, brick (b2 B1 + b1) B0 + b0
"""
import numpy as np

import query_ref as Q

f32 = np.float32
SLOTS, ROWS = 16, 17
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def spec(origin, cell, n):
    cell = (cell,) * 3 if isinstance(cell, (int, float)) else tuple(cell)
    n = (n,) * 3 if isinstance(n, int) else tuple(int(x) for x in n)
    return tuple(origin), cell, n


def axes(origin, cell, n):
    """The sample coordinates per axis: RN(origin + RN(((float)i + 0.5f) cell))."""
    return [(f32(origin[c]) + ((np.arange(n[c]).astype(f32) + f32(0.5)) * f32(cell[c])).astype(f32))
            .astype(f32) for c in range(3)]


def points(origin, cell, n):
    ax = axes(origin, cell, n)
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1).astype(f32)


def row_of(mask, n):
    """The 16 slots of the samples set in `mask` [i2, i1, i0]."""
    r = np.zeros(SLOTS, dtype=np.int64)
    r[10:13] = n
    r[13:16] = -1
    i2, i1, i0 = np.nonzero(mask)
    if len(i0) == 0:
        return r
    idx = [i0.astype(np.int64), i1.astype(np.int64), i2.astype(np.int64)]
    r[0] = len(i0)
    for c in range(3):
        r[1 + c] = idx[c].sum()
        r[10 + c] = idx[c].min()
        r[13 + c] = idx[c].max()
    for s, (c, d) in enumerate(PAIRS):
        r[4 + s] = (idx[c] * idx[d]).sum()
    return r


def bricks_of(inside, n):
    """Per-brick facts of an inside array: (mixed, all-inside, bricks in all) --
    bricks holding both inside and outside samples, and bricks whose samples are
    all inside."""
    nb = [(n[c] + 7) // 8 for c in range(3)]
    mixed = full = 0
    for b2 in range(nb[2]):
        for b1 in range(nb[1]):
            for b0 in range(nb[0]):
                blk = inside[8 * b2:8 * b2 + 8, 8 * b1:8 * b1 + 8, 8 * b0:8 * b0 + 8]
                k = int(blk.sum())
                full += k == blk.size
                mixed += 0 < k < blk.size
    return mixed, full, int(np.prod(nb))


def measure(frame, origin, cell, n, iso=0.0, owners=False):
    """The reference of sdf_measure in exact precision: dict of rows ((1 or 17,
    16) int64), bricks (mixed, all-inside, all), min_abs_w (the sample value
    closest to a change of sign), inside (the bool array) and, with owners,
    min_owner_gap (the closest owner decision over the inside samples)."""
    origin, cell, n = spec(origin, cell, n)
    P = points(origin, cell, n)
    with np.errstate(all="ignore"):
        w = (Q.scene_sdf(frame, P) - f32(iso)).astype(f32)
    inside = (w < 0).reshape(n[2], n[1], n[0])             # a NaN or a zero is outside
    rows = [row_of(inside, n)]
    r = {"bricks": bricks_of(inside, n), "inside": inside}
    with np.errstate(all="ignore"):
        r["min_abs_w"] = float(np.nanmin(np.abs(w)))
    if owners:
        sel = np.nonzero(inside.ravel())[0]
        own = np.full(inside.size, -1, dtype=np.int32)
        gap = np.inf
        if len(sel):
            own[sel], g = Q.owner(frame, P[sel])
            gap = float(g.min())
        own = own.reshape(inside.shape)
        rows += [row_of(own == k, n) for k in range(ROWS - 1)]
        r["min_owner_gap"] = gap
    r["rows"] = np.stack(rows)
    return r
