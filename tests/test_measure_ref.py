"""tests/measure_ref.py, the NumPy reference of sdf_measure, against closed
forms (CPU only), and the preconditions of the fast-precision GPU cases: the
reference's samples stay away from a change of sign by more than the bound the
project holds fast distances to."""
import math

import numpy as np
import pytest

import fast_paths as FP
import measure_ref as MR
from cases import C4_GRID
from cases import query_frame as frame_of
from sdf3d_amd import abi, renderer as R, scenes
from sdf3d_amd.measure import Measure


def as_measure(ref, origin, cell, n):
    g = R.grid(origin, cell, n)          # the grid's own fp32 values
    return Measure(ref["rows"], (0, 0, ref["bricks"][2], 0), tuple(g.origin), tuple(g.cell), tuple(g.n))


def test_a_box_on_cell_faces_is_exact():
    """A box whose faces lie on cell faces (every number dyadic): 8 x 8 x 6 cells
    inside, so volume, centroid and inertia are the box's own up to fp64
    rounding -- the variance of k consecutive integers is (k^2 - 1) / 12, and
    the cells' own cell^2 / 12 completes it to (k cell)^2 / 12."""
    f = scenes.config("C1", 64, 36)
    centre, half = (0.25, 0.5, -0.125), (0.5, 0.25, 0.375)
    scenes._prim(f.scene, 0, abi.PRIM_BOX, abi.OP_UNION, 0.0, *centre, *half)
    origin, cell, n = (-0.5, 0.0, -0.75), (0.125, 0.0625, 0.125), (12, 14, 12)
    ref = MR.measure(f, origin, cell, n, owners=True)
    row = ref["rows"][0]
    assert row[0] == 8 * 8 * 6
    assert row[10:13].tolist() == [2, 4, 2] and row[13:16].tolist() == [9, 11, 7]
    assert np.array_equal(ref["rows"][1], row) and (ref["rows"][2:, 0] == 0).all()
    assert ref["bricks"] == (4, 0, 8)     # cells 2..9, 4..11, 2..7: none in the bricks of i2 >= 8
    m = as_measure(ref, origin, cell, n)
    a, b, c = (2 * h for h in half)
    assert m.volume() == a * b * c
    assert np.array_equal(m.centroid(), np.array(centre))
    lo, hi = m.bounds()
    assert np.array_equal(lo, np.array(centre) - half) and np.array_equal(hi, np.array(centre) + half)
    mass = 2.0 * a * b * c
    want = mass / 12 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b])
    assert np.allclose(m.inertia(2.0), want, rtol=1e-13, atol=1e-16)
    assert np.allclose(m.inertia(densities=[2.0]), want, rtol=1e-13, atol=1e-16)


def test_a_sphere_within_its_rigorous_bounds():
    """C1's sphere (r = 0.2 at (0, 0.4, 0)) on 32^3 cells of 1 / 64.  The solid of
    the measure is the union S of the cells whose centre is inside; S and the
    ball B differ only inside cells with corners of both signs, so

      |V_S - V_B|  <=  mixed * cell volume.

    Ixx: about the ball's centre c the two integrals of rho^2 = y^2 + z^2 differ
    by at most the mixed cells' volume times the largest rho^2 in them, (r +
    sqrt 3 cell)^2; moving the axis from c to S's own centroid lowers Ixx_S by
    M_S d^2 with d the centroids' distance in the y-z plane.  So

      |Ixx_S - Ixx_B|  <=  mixed * cell volume * (r + sqrt 3 cell)^2 + M_S d^2.

    Measured on the CPU oracle: 3,070 mixed cells of 32,768; volume 0.033500671
    against 0.033510322, relative error 2.88e-4 (bound 0.35); centroid within
    2.6e-4 of the centre (half a cell: 7.8e-3); Ixx 5.373635e-4 against
    5.361651e-4, relative error 2.2e-3 (bound 1.13)."""
    f = frame_of("C1")
    origin, cell, n = (-0.2513, 0.1479, -0.2491), 1.0 / 64, 32
    centre, r = np.array([0.0, 0.4, 0.0]), 0.2
    ref = MR.measure(f, origin, cell, n)
    m = as_measure(ref, origin, cell, n)
    # corners of both signs, in fp64 on the real lattice
    ax = [m.origin[c] + np.arange(n + 1) * m.cell[c] for c in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    inside = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) < r
    cnt = sum(inside[k >> 2:(k >> 2) + n, (k >> 1 & 1):(k >> 1 & 1) + n, (k & 1):(k & 1) + n].astype(int)
              for k in range(8))
    mixed = int(((cnt > 0) & (cnt < 8)).sum())
    cv = m.cell_volume
    vol, want = m.volume(), 4.0 / 3.0 * math.pi * r ** 3
    off = m.centroid() - centre
    ixx, ixx_want = m.inertia()[0, 0], 0.4 * want * r * r
    ixx_bound = mixed * cv * (r + math.sqrt(3) * cell) ** 2 + vol * (off[1] ** 2 + off[2] ** 2)
    print(f"mixed {mixed} of {n ** 3}; volume {vol:.9f} against {want:.9f}: relative error "
          f"{abs(vol - want) / want:.3e}, bound {mixed * cv / want:.3e}; centroid off by "
          f"{np.abs(off).max():.3e}; Ixx {ixx:.6e} against {ixx_want:.6e}: relative error "
          f"{abs(ixx - ixx_want) / ixx_want:.3e}, bound {ixx_bound / ixx_want:.3e}")
    assert 0 < mixed < n ** 3 // 8
    assert abs(vol - want) <= mixed * cv
    assert np.abs(off).max() <= cell / 2
    assert abs(ixx - ixx_want) <= ixx_bound
    lo, hi = m.bounds()
    assert np.all(lo <= centre - r + cell) and np.all(hi >= centre + r - cell)
    assert np.all(lo >= centre - r - cell) and np.all(hi <= centre + r + cell)


def test_rows_and_brick_facts_are_consistent():
    """On C4's mesh grid: the owner rows add up to row 0 and envelop it; the brick
    facts count what they say."""
    f = frame_of("C4")
    ref = MR.measure(f, *C4_GRID, owners=True)
    rows = ref["rows"]
    assert rows.shape == (MR.ROWS, MR.SLOTS) and rows.dtype == np.int64
    assert np.array_equal(rows[1:, :10].sum(axis=0), rows[0, :10]) and rows[0, 0] > 0
    assert np.array_equal(rows[1:, 10:13].min(axis=0), rows[0, 10:13])
    assert np.array_equal(rows[1:, 13:16].max(axis=0), rows[0, 13:16])
    assert (rows[1 + f.scene.count:, 0] == 0).all()
    mixed, full, total = ref["bricks"]
    assert total == 3 * 2 * 3 and 0 < mixed <= total and mixed + full <= total
    assert np.array_equal(MR.measure(f, *C4_GRID)["rows"], rows[:1])
    # iso moves the surface outwards: more samples inside
    assert MR.measure(f, *C4_GRID, iso=0.05)["rows"][0, 0] > rows[0, 0]


C1_OFF = ((-0.31, 0.13, -0.29), (0.05, 0.06, 0.055), (12, 10, 11))
C4_OFF = ((-1.094, -0.086, -0.99), *C4_GRID[1:])
# the fast cases of tests/test_gpu_measure.py: (kind, grid, min |w| measured on the CPU oracle)
FAST_GRIDS = {
    "C1": ("C1", C1_OFF, 2.0e-4),
    "C4": ("C4", C4_OFF, 1.17e-3),
    "C4-carved": ("C4-carved", C4_OFF, 1.17e-3),
    "J0": ("J0", C4_GRID, 5.7e-3),
    "J4": ("J4", C4_GRID, 1.1e-4),
    "J6": ("J6", C4_GRID, 2.0e-3),
}


@pytest.mark.parametrize("case", list(FAST_GRIDS))
def test_fast_cases_stay_away_from_a_change_of_sign(case):
    kind, grid, measured = FAST_GRIDS[case]
    ref = MR.measure(frame_of(kind), *grid)
    print(f"{case}: min |w| {ref['min_abs_w']:.4e}")
    assert ref["min_abs_w"] > FP.FAST_BOUND_T
    assert 0.97 * measured <= ref["min_abs_w"] <= 1.03 * measured     # the figure as recorded


def test_c4_on_its_mesh_grid_is_no_fast_case():
    assert MR.measure(frame_of("C4"), *C4_GRID)["min_abs_w"] < FP.FAST_BOUND_T
