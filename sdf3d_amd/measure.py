"""What sdf_measure's integer rows mean (include/sdf_abi.h "Measures", host
conversion): volume, mass, centroid, covariance, inertia tensor and bounds in
fp64 over the real-valued lattice coordinates origin + (i + 1/2) cell.  NumPy
only: no GPU and no library needed, so rows from any source convert.

A row is 16 int64 over a set of inside samples: N, S (3), Q (00, 11, 22, 01, 02,
12), lo (3), hi (3); an empty set has N = 0, lo = n and hi = -1."""
from typing import NamedTuple, Optional

import numpy as np

SLOTS = 16
ROWS = 17          # row 0, then a row per primitive
_Q = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # slots 4 .. 9


def empty_row(n):
    """The row of the empty set on a grid of n = (n0, n1, n2) samples."""
    r = np.zeros(SLOTS, dtype=np.int64)
    r[10:13] = n
    r[13:16] = -1
    return r


class Moments(NamedTuple):
    """Weighted raw moments of a set: m0 = sum of weights, m1[c] = sum of w i_c,
    m2[c, d] = sum of w i_c i_d (fp64, symmetric)."""
    m0: float
    m1: np.ndarray
    m2: np.ndarray


class Measure:
    """The rows and counts of one sdf_measure call on one grid.

    `rows` is (1, 16) or, with owners, (17, 16) int64; `counts` the call's four
    numbers (bricks evaluated, bricks in closed form, bricks in all, 0);
    `origin`, `cell` and `n` the grid.  Every helper works on row 0, the whole
    solid, unless `densities` (a weight per primitive; owners needed) or a
    `select`-ed row says otherwise."""

    def __init__(self, rows, counts, origin, cell, n):
        rows = np.asarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[1] != SLOTS or rows.shape[0] not in (1, ROWS):
            raise ValueError(f"rows must be (1, {SLOTS}) or ({ROWS}, {SLOTS}) int64")
        self.rows = rows
        self.counts = tuple(int(x) for x in counts)
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        cell = (cell,) * 3 if isinstance(cell, (int, float)) else cell
        n = (n,) * 3 if isinstance(n, (int, np.integer)) else n
        self.cell = np.asarray(cell, dtype=np.float64).reshape(3)
        self.n = tuple(int(x) for x in n)

    @property
    def owners(self) -> bool:
        return self.rows.shape[0] == ROWS

    # ---- raw moments ------------------------------------------------------------------
    @staticmethod
    def _of_row(row, weight=1.0) -> Moments:
        m2 = np.zeros((3, 3))
        for s, (c, d) in enumerate(_Q):
            m2[c, d] = m2[d, c] = float(row[4 + s])
        return Moments(weight * float(row[0]), weight * row[1:4].astype(np.float64), weight * m2)

    def moments(self, densities=None) -> Moments:
        """Row 0's raw moments, or with `densities` sum_k rho_k (N_k, S_k, Q_k)
        over the owner rows (primitives beyond the list weigh 0)."""
        if densities is None:
            return self._of_row(self.rows[0])
        if not self.owners:
            raise ValueError("densities need the owner rows (owners=True)")
        rho = np.zeros(ROWS - 1)
        d = np.asarray(densities, dtype=np.float64).reshape(-1)
        if len(d) > ROWS - 1:
            raise ValueError(f"at most {ROWS - 1} densities")
        rho[:len(d)] = d
        m0, m1, m2 = 0.0, np.zeros(3), np.zeros((3, 3))
        for k in range(ROWS - 1):
            m = self._of_row(self.rows[1 + k], rho[k])
            m0, m1, m2 = m0 + m.m0, m1 + m.m1, m2 + m.m2
        return Moments(m0, m1, m2)

    # ---- the measures -----------------------------------------------------------------
    @property
    def cell_volume(self) -> float:
        return float(np.prod(self.cell))

    def volume(self) -> float:
        """N c0 c1 c2 of row 0."""
        return float(self.rows[0, 0]) * self.cell_volume

    def mass(self, densities) -> float:
        """sum_k rho_k N_k c0 c1 c2; a scalar density weighs row 0."""
        if np.ndim(densities) == 0:
            return float(densities) * self.volume()
        return self.moments(densities).m0 * self.cell_volume

    def centroid(self, densities=None) -> np.ndarray:
        """origin + (S / N + 1/2) cell; NaN for an empty (or weightless) set."""
        m = self.moments(densities)
        with np.errstate(all="ignore"):
            return self.origin + (m.m1 / m.m0 + 0.5) * self.cell

    def covariance(self, densities=None) -> np.ndarray:
        """C_cd = (Q_cd / N - (S_c / N)(S_d / N)) c_c c_d + [c = d] c_c^2 / 12: the
        second central moments per unit mass of the union of the cells."""
        m = self.moments(densities)
        with np.errstate(all="ignore"):
            mean = m.m1 / m.m0
            cov = (m.m2 / m.m0 - np.outer(mean, mean)) * np.outer(self.cell, self.cell)
        return cov + np.diag(self.cell ** 2 / 12.0)

    def inertia(self, density: float = 1.0, densities=None) -> np.ndarray:
        """The inertia tensor about the centroid, mass (tr(C) Id - C); the mass is
        density * volume, or mass(densities)."""
        c = self.covariance(densities)
        mass = density * self.volume() if densities is None else self.mass(densities)
        return mass * (np.trace(c) * np.eye(3) - c)

    def bounds(self) -> Optional[tuple]:
        """(lower, upper) corners of the cells row 0 occupies: origin + lo cell and
        origin + (hi + 1) cell; None for an empty set."""
        r = self.rows[0]
        if r[0] == 0:
            return None
        return (self.origin + r[10:13] * self.cell, self.origin + (r[13:16] + 1) * self.cell)

    def select(self, prims) -> "Measure":
        """The measure whose row 0 combines the owner rows of `prims` (sums; min
        and max for lo and hi) -- everything but the ground plane, say.  It has no
        owner rows of its own."""
        if not self.owners:
            raise ValueError("select needs the owner rows (owners=True)")
        row = empty_row(self.n)
        for k in sorted(set(int(p) for p in prims)):
            if not 0 <= k < ROWS - 1:
                raise ValueError(f"no primitive {k}")
            r = self.rows[1 + k]
            row[:10] += r[:10]
            row[10:13] = np.minimum(row[10:13], r[10:13])
            row[13:16] = np.maximum(row[13:16], r[13:16])
        return Measure(row[None, :], self.counts, self.origin, self.cell, self.n)


def fit_grid(bounds, cells: int, margin: int = 1):
    """(origin, cell, n) of cubic cells around the box `bounds` = (lower, upper):
    the longest side takes `cells` cells, the others as many as cover them, and
    `margin` cells are added on every side -- so that a coarse measure's bounds
    place the grid of a fine mesh with the surface inside it."""
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    ext = hi - lo
    if cells < 1 or margin < 0 or not np.all(np.isfinite(ext)) or not ext.max() > 0 or ext.min() < 0:
        raise ValueError("fit_grid needs a finite box with a positive side, cells >= 1, margin >= 0")
    cell = float(ext.max()) / cells
    # a side that is a whole number of cells takes that many, whatever the division rounded to
    inner = np.maximum(1, np.ceil(ext / cell * (1.0 - 1e-12)).astype(np.int64))
    n = tuple(int(x) + 2 * margin for x in inner)
    origin = tuple(float(x) for x in lo - margin * cell)
    return origin, cell, n
