"""sdf_measure at the C-ABI boundary, without a GPU (include/sdf_abi.h
"Measures"): symbols, every documented error decided before any device call,
the workspace formula, and the fp64 helpers of sdf3d_amd/measure.py on
hand-made rows."""
import ctypes as C
import math

import numpy as np
import pytest

from sdf3d_amd import abi, fit_grid, renderer as R, scenes
from sdf3d_amd.measure import Measure, empty_row

INVALID = abi.SDF_E_INVALID_ARG
# A 16-byte aligned address that is never dereferenced: it goes only to calls that are refused
# before any device call.  Arguments that are valid throughout go to sdf_validate_measure alone.
FAKE = C.c_void_p(1 << 20)
OWN = abi.MEASURE_OWNERS


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame():
    return scenes.config("C4", 64, 36)


def good_grid():
    return R.grid((-1.13, -0.11, -1.02), (0.12, 0.08, 0.11), (19, 11, 17))


def validate(lib, f, g, flags=0):
    return lib.sdf_validate_measure(C.byref(f.scene), C.byref(f.params), C.byref(g), flags)


def calls(lib, f, g, flags=0, ws=FAKE, nbytes=None, moments=FAKE, counts=FAKE):
    """(validate, measure) return codes for one set of arguments, of which at
    least one is invalid: sdf_measure must refuse them before it touches a
    device or a buffer."""
    gp = C.byref(g) if g is not None else None
    if nbytes is None:
        nbytes = max(int(lib.sdf_measure_workspace_bytes(gp, flags)), 0)
    return (lib.sdf_validate_measure(C.byref(f.scene), C.byref(f.params), gp, flags),
            lib.sdf_measure(C.byref(f.scene), C.byref(f.params), gp, flags, ws, nbytes, moments,
                            counts, None))


def test_symbols_and_constants(lib):
    for name, nargs in (("sdf_validate_measure", 4), ("sdf_measure_workspace_bytes", 2),
                        ("sdf_measure", 9)):
        assert hasattr(lib, name), name
        assert len(abi.SIGNATURES[name][1]) == nargs
    assert abi.SIGNATURES["sdf_measure_workspace_bytes"][0] is C.c_int64
    assert (abi.MEASURE_OWNERS, abi.MEASURE_SLOTS, abi.MEASURE_ROWS) == (1, 16, 1 + abi.SDF_MAX_PRIMS)
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


def test_validator_accepts_every_config(lib):
    g = good_grid()
    for name in scenes.CONFIGS:
        f = scenes.config(name)
        for flags in (0, OWN):
            assert validate(lib, f, g, flags) == abi.SDF_OK
    g.flags, g.iso = abi.MESH_DENSE, 0.05
    assert validate(lib, frame(), g) == abi.SDF_OK
    g = R.grid((0, 0, 0), 1e-4, (65536, 1, 1))                 # the largest axis
    assert validate(lib, frame(), g) == abi.SDF_OK


def bad_grids():
    def edit(**kw):
        g = good_grid()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        return g
    inf, nan = math.inf, math.nan
    return {
        # what sdf_validate_mesh rejects
        "n zero": edit(n=(1, 0)), "n negative": edit(n=(2, -3)),
        "2^30 + 1 points": R.grid((0, 0, 0), 0.001, (1023, 1023, 1024)),
        "cell zero": edit(cell=(0, 0.0)), "cell nan": edit(cell=(0, nan)),
        "origin inf": edit(origin=(0, -inf)), "iso nan": edit(iso=nan),
        "far corner beyond 1e15": R.grid((9.9e14, 0, 0), (1e12, 1.0, 1.0), (19, 2, 2)),
        "unknown grid flag": edit(flags=2), "reserved": edit(reserved=1),
        # and the measure's own limit, on each axis
        "n0 = 65537": R.grid((0, 0, 0), 1e-4, (65537, 1, 1)),
        "n1 = 65537": R.grid((0, 0, 0), 1e-4, (1, 65537, 1)),
        "n2 = 65537": R.grid((0, 0, 0), 1e-4, (1, 1, 65537)),
    }


@pytest.mark.parametrize("what", list(bad_grids()))
def test_bad_grids_are_refused(lib, what):
    g = bad_grids()[what]
    for flags in (0, OWN):
        assert calls(lib, frame(), g, flags) == (INVALID, INVALID)
        assert lib.sdf_measure_workspace_bytes(C.byref(g), flags) == INVALID


def test_the_mesh_accepts_what_the_axis_limit_refuses(lib):
    f, g = frame(), R.grid((0, 0, 0), 1e-4, (65537, 1, 1))
    assert lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g)) == abi.SDF_OK


def test_flags_null_arguments_and_buffers(lib):
    f, g = frame(), good_grid()
    for flags in (2, 3, -1, 0x100):
        assert calls(lib, f, g, flags, nbytes=1 << 20) == (INVALID, INVALID)
        assert lib.sdf_measure_workspace_bytes(C.byref(g), flags) == INVALID
    assert calls(lib, f, None) == (INVALID, INVALID)
    assert lib.sdf_measure_workspace_bytes(None, 0) == INVALID
    assert lib.sdf_validate_measure(None, C.byref(f.params), C.byref(g), 0) == INVALID
    assert lib.sdf_validate_measure(C.byref(f.scene), None, C.byref(g), 0) == INVALID
    for flags in (0, OWN):
        need = int(lib.sdf_measure_workspace_bytes(C.byref(g), flags))
        assert calls(lib, f, g, flags, moments=None)[1] == INVALID
        assert calls(lib, f, g, flags, counts=None)[1] == INVALID
        assert calls(lib, f, g, flags, ws=None)[1] == INVALID
        assert calls(lib, f, g, flags, ws=C.c_void_p((1 << 20) + 8))[1] == INVALID   # misaligned
        assert calls(lib, f, g, flags, nbytes=need - 1)[1] == INVALID
    # the workspace of a call without owners is too small for one with them
    assert calls(lib, f, g, OWN, nbytes=int(lib.sdf_measure_workspace_bytes(C.byref(g), 0)))[1] == INVALID


def test_what_the_query_validator_rejects(lib):
    g = good_grid()
    for field, value in (("normal_mode", 7), ("precision", 9)):
        f = frame()
        setattr(f.params, field, value)
        assert calls(lib, f, g) == (INVALID, INVALID)
    f = frame()
    f.scene.prims[1].kind = 99
    assert calls(lib, f, g) == (INVALID, INVALID)


def test_workspace_formula(lib):
    def need(n, flags):
        return int(lib.sdf_measure_workspace_bytes(C.byref(R.grid((0, 0, 0), 0.01, n)), flags))

    def formula(n, flags):
        b = math.prod((x + 7) // 8 for x in n)
        rows = abi.MEASURE_ROWS if flags else 1
        return 8 * min(b, abi.MEASURE_MAX_BLOCKS) * (16 * rows + 4)
    for n in ((1, 1, 1), (8, 8, 8), (9, 8, 8), (19, 11, 17), (128, 128, 128), (65536, 1, 1),
              (512, 512, 512)):
        for flags in (0, OWN):
            assert need(n, flags) == formula(n, flags), (n, flags)
    # capped: 512^3 cells need what 128^3 do, below 1 MB without owners and 10 MB with
    assert need((512,) * 3, 0) == need((128,) * 3, 0) < 1 << 20
    assert need((512,) * 3, OWN) < 10 << 20


# ---- the helpers on hand-made rows ---------------------------------------------------------

def row_of(idx, n):
    """The row of the samples `idx` (k, 3) by the definition, in Python integers."""
    r = empty_row(n)
    idx = [tuple(int(x) for x in i) for i in idx]
    r[0] = len(idx)
    for c in range(3):
        r[1 + c] = sum(i[c] for i in idx)
    for s, (c, d) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        r[4 + s] = sum(i[c] * i[d] for i in idx)
    if idx:
        r[10:13] = [min(i[c] for i in idx) for c in range(3)]
        r[13:16] = [max(i[c] for i in idx) for c in range(3)]
    return r


ORIGIN, CELL, N = (-1.0, 0.5, 2.0), (0.5, 0.25, 0.125), (8, 6, 5)


def test_empty_set():
    m = Measure(empty_row(N)[None], (0, 0, 1, 0), ORIGIN, CELL, N)
    assert m.volume() == 0.0 and m.bounds() is None and not m.owners
    assert np.isnan(m.centroid()).all() and m.mass(2.0) == 0.0
    assert m.counts == (0, 0, 1, 0)


def test_one_sample():
    i = (3, 2, 4)
    m = Measure(row_of([i], N)[None], (1, 0, 1, 0), ORIGIN, CELL, N)
    cell = np.array(CELL)
    assert m.volume() == 0.5 * 0.25 * 0.125
    assert np.array_equal(m.centroid(), np.array(ORIGIN) + (np.array(i) + 0.5) * cell)
    # one cell: the covariance of a uniform box, cell^2 / 12 on the diagonal
    assert np.allclose(m.covariance(), np.diag(cell ** 2 / 12), rtol=0, atol=1e-15)
    lo, hi = m.bounds()
    assert np.array_equal(lo, np.array(ORIGIN) + np.array(i) * cell) and np.array_equal(hi, lo + cell)
    # the inertia of a box of sides a, b, c and mass M about its centre
    a, b, c = CELL
    M = 3.0 * m.volume()
    assert np.allclose(m.inertia(3.0), M / 12 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b]),
                       rtol=1e-12, atol=0)


def owner_measure():
    sets = {0: [(0, 0, 0), (1, 0, 0), (7, 5, 4)], 2: [(3, 2, 1), (3, 3, 1)], 5: [(6, 1, 2)]}
    rows = [row_of(sum(sets.values(), []), N)] + [row_of(sets.get(k, []), N) for k in range(16)]
    return Measure(np.stack(rows), (1, 0, 1, 0), ORIGIN, CELL, N), sets


def test_densities_and_select():
    m, sets = owner_measure()
    assert m.owners and m.volume() == 6 * m.cell_volume
    rho = [2.0, 9.0, 0.5, 0.0, 0.0, 4.0]
    assert m.mass(rho) == (2.0 * 3 + 0.5 * 2 + 4.0 * 1) * m.cell_volume
    # the weighted centroid from the samples themselves
    pts = [(np.array(ORIGIN) + (np.array(i) + 0.5) * np.array(CELL), rho[k])
           for k, s in sets.items() for i in s]
    want = sum(w * p for p, w in pts) / sum(w for _, w in pts)
    assert np.allclose(m.centroid(rho), want, rtol=1e-14, atol=1e-14)
    # weighted covariance: the point masses' plus the cells' own cell^2 / 12
    d = np.stack([p - want for p, _ in pts])
    w = np.array([x for _, x in pts])
    cov = (d * w[:, None]).T @ d / w.sum() + np.diag(np.array(CELL) ** 2 / 12)
    assert np.allclose(m.covariance(rho), cov, rtol=1e-12, atol=1e-14)
    assert np.allclose(m.inertia(densities=rho), m.mass(rho) * (np.trace(cov) * np.eye(3) - cov),
                       rtol=1e-12, atol=1e-14)
    # unit densities are row 0
    assert np.allclose(m.centroid([1.0] * 16), m.centroid(), rtol=1e-15, atol=0)
    # select: everything but primitive 0
    s = m.select([2, 5, 5, 9])
    assert np.array_equal(s.rows[0], row_of(sets[2] + sets[5], N)) and not s.owners
    assert s.volume() == 3 * m.cell_volume
    assert np.array_equal(m.select(range(16)).rows[0], m.rows[0])
    assert m.select([9]).bounds() is None
    with pytest.raises(ValueError):
        m.select([16])
    with pytest.raises(ValueError):
        s.select([0])
    with pytest.raises(ValueError):
        s.mass([1.0, 2.0])
    with pytest.raises(ValueError):
        Measure(np.zeros((2, 16), dtype=np.int64), (0, 0, 0, 0), ORIGIN, CELL, N)


def test_fit_grid():
    origin, cell, n = fit_grid(((-1.0, 0.0, 0.25), (1.0, 0.5, 0.75)), 64)
    assert cell == 2.0 / 64 and n == (66, 18, 18)
    assert origin == (-1.0 - cell, 0.0 - cell, 0.25 - cell)
    # the grid covers the box with its margin, in cubic cells
    for c, (lo, hi) in enumerate(zip((-1.0, 0.0, 0.25), (1.0, 0.5, 0.75))):
        assert origin[c] <= lo - cell * (1 - 1e-12) and origin[c] + n[c] * cell >= hi + cell * (1 - 1e-12)
    origin, cell, n = fit_grid(((0.0, 0.0, 0.0), (0.3, 0.1, 0.0)), 3, margin=0)
    assert n == (3, 1, 1) and origin == (0.0, 0.0, 0.0) and math.isclose(cell, 0.1)
    m, _ = owner_measure()
    o, c, n = fit_grid(m.bounds(), 32, margin=2)
    assert max(n) == 36 and all(o[k] < m.bounds()[0][k] for k in range(3))
    for bad in (((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (math.inf, 1, 1))):
        with pytest.raises(ValueError):
            fit_grid(bad, 8)
    with pytest.raises(ValueError):
        fit_grid(((0, 0, 0), (1, 1, 1)), 0)
