"""GPU tests of sdf_measure (include/sdf_abi.h "Measures") against
tests/measure_ref.py, the NumPy reference over the CPU oracle.  Every output is
an exact integer sum, so every slot of every row equals the reference: in exact
precision on every dispatch path, with and without the owner rows, with and
without brick skipping; in fast precision on the grids whose samples stay away
from a change of sign by more than the bound the project holds fast distances
to (tests/test_measure_ref.py asserts that of the reference).

Grids: partial bricks on every axis, several bricks per axis, more bricks than
the launch has workgroups, sub-second references.  `moments` and `counts` stand
in fenced buffers (gpu_support.out_buf), whose guard rows must survive.  A
case's GPU rows and its reference are computed once."""
import ctypes as C
import json

import numpy as np
import pytest

import fast_paths as FP
import measure_ref as MR
from cases import C4_GRID, JIT_SEEDS
from cases import query_frame as frame_of
from gpu_support import out_buf, ptr, sdf_main, stream_of, taken
from sdf3d_amd import abi, measure as MS, renderer as R

pytestmark = pytest.mark.gpu

FAST = abi.PRECISION_FAST
OWN = abi.MEASURE_OWNERS
C1_OFF = ((-0.31, 0.13, -0.29), (0.05, 0.06, 0.055), (12, 10, 11))
C4_OFF = ((-1.094, -0.086, -0.99), *C4_GRID[1:])
# case -> (scene kind of cases.query_frame, origin, cell, n, iso)
CASES = {
    "REF": ("REF", *C4_GRID, 0.0),
    "C1": ("C1", *C4_GRID, 0.0),
    "C4": ("C4", *C4_GRID, 0.0),
    "C4-generic": ("C4-generic", *C4_GRID, 0.0),
    "C4-unculled": ("C4-unculled", *C4_GRID, 0.0),
    "C4-carved": ("C4-carved", *C4_GRID, 0.0),
    "J0": ("J0", *C4_GRID, 0.0),
    "J4": ("J4", *C4_GRID, 0.0),
    "J6": ("J6", *C4_GRID, 0.0),
    "C1-iso": ("C1", *C1_OFF, 0.05),
    "C5": ("C5", (-0.61, -0.32, -0.59), (0.05, 0.05, 0.05), (24, 25, 23), 0.0),
}
# the fast cases: tests/test_measure_ref.py holds their min |w| above FAST_BOUND_T
FAST_CASES = {
    "C1": ("C1", *C1_OFF, 0.0),
    "C4": ("C4", *C4_OFF, 0.0),
    "C4-carved": ("C4-carved", *C4_OFF, 0.0),
    "J0": ("J0", *C4_GRID, 0.0),
    "J4": ("J4", *C4_GRID, 0.0),
    "J6": ("J6", *C4_GRID, 0.0),
}
FINE = ("C4", (-1.01, -0.97, -1.02), (0.04, 0.04, 0.04), (50, 43, 42), 0.0)
_ref, _exact = {}, {}


def run(rd, f, spec, flags=0, dense=False, fill=None):
    """sdf_measure through the C ABI into fenced buffers: (rows (R, 16) int64,
    counts (4,))."""
    torch = rd.torch
    g = R.grid(*spec, dense=dense)
    nbytes = int(rd.lib.sdf_measure_workspace_bytes(C.byref(g), flags))
    assert nbytes > 0, "sdf_measure_workspace_bytes gave no size"
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=rd.device)
    if fill is not None:
        ws.fill_(fill)
    rows = abi.MEASURE_ROWS if flags & OWN else 1
    bm = out_buf(rd, rows, abi.MEASURE_SLOTS, torch.int64)
    bc = out_buf(rd, 4, 1, torch.int64)
    rc = rd.lib.sdf_measure(C.byref(f.scene), C.byref(f.params), C.byref(g), flags, ptr(ws), nbytes,
                            ptr(bm), ptr(bc), stream_of(rd))
    abi.check(rc, "sdf_measure")
    torch.cuda.synchronize()
    return taken(rd, bm), tuple(int(x) for x in taken(rd, bc))


def reference(key, kind, spec):
    """measure_ref.measure with owners of the exact frame `kind` on `spec`, once."""
    if key not in _ref:
        _ref[key] = MR.measure(frame_of(kind), *spec, owners=True)
        _ref[key]["rows"].setflags(write=False)
    return _ref[key]


def compiled(kind):
    return FP.jit_on() and (kind in JIT_SEEDS or kind in FP.JIT)


def exact_run(rd, case, flags):
    """(rows, counts, reference, compilations of the first call and of a second)
    of `case` in exact precision, computed once; two calls give equal bits."""
    if (case, flags) not in _exact:
        kind, *spec = CASES[case] if case != "FINE" else FINE
        f = frame_of(kind)
        n0 = rd.lib.sdf_jit_count()
        rows, counts = run(rd, f, spec, flags)
        n1 = rd.lib.sdf_jit_count()
        again, counts2 = run(rd, f, spec, flags)
        n2 = rd.lib.sdf_jit_count()
        assert np.array_equal(rows, again) and counts == counts2, f"{case}: two calls differ"
        _exact[case, flags] = (rows, counts, reference(("exact", case), kind, spec), n1 - n0, n2 - n1)
    return _exact[case, flags]


def want_rows(ref, flags):
    return ref["rows"] if flags & OWN else ref["rows"][:1]


# 1. exact precision -------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, OWN], ids=["all", "owners"])
@pytest.mark.parametrize("case", list(CASES))
def test_exact_rows_equal_the_reference(renderer, case, flags):
    """Every slot of every row and counts[2] equal the reference; a run-time
    specialised scene compiles exactly one kernel per flag, whatever ran before,
    and none on the second call."""
    rows, counts, ref, jit_first, jit_second = exact_run(renderer, case, flags)
    want = want_rows(ref, flags)
    print(f"{case}: row 0 {rows[0].tolist()} counts {counts} reference bricks {ref['bricks']} "
          f"slots differing {int((rows != want).sum())}")
    assert rows.shape == want.shape and np.array_equal(rows, want)
    assert counts[2] == ref["bricks"][2] and counts[3] == 0
    assert counts[0] + counts[1] <= counts[2] and counts[0] >= ref["bricks"][0]
    assert counts[1] <= ref["bricks"][1] and (not flags or counts[1] == 0)
    assert (jit_first, jit_second) == (1 if compiled(CASES[case][0]) else 0, 0)
    if case == "C5":
        assert counts[0] == counts[2]       # no Lipschitz bound: always dense


# 2. skipping bricks changes nothing -----------------------------------------------
def test_skip_equals_dense(renderer):
    """C4 on 50 x 43 x 42 cells (252 bricks, 90,300 samples): every slot matches
    with and without SDF_MESH_DENSE, and the reference; bricks are skipped, and
    taken in closed form, only without."""
    rows, counts, ref, _, _ = exact_run(renderer, "FINE", 0)
    kind, *spec = FINE
    dense, dcounts = run(renderer, frame_of(kind), spec, dense=True)
    print(f"C4 fine: counts {counts} dense {dcounts} reference bricks {ref['bricks']}")
    assert np.array_equal(rows, dense) and np.array_equal(rows, ref["rows"][:1])
    assert counts[2] == dcounts[2] == ref["bricks"][2] == 252
    assert dcounts[0] == dcounts[2] and dcounts[1] == 0
    assert counts[1] > 0 and counts[0] + counts[1] < counts[2]
    assert counts[0] >= ref["bricks"][0]
    assert counts[1] <= ref["bricks"][1]


def test_skip_with_owners_evaluates_the_inside_bricks(renderer):
    rows, counts, ref, _, _ = exact_run(renderer, "FINE", OWN)
    print(f"C4 fine with owners: counts {counts}")
    assert counts[1] == 0 and counts[0] < counts[2]
    assert np.array_equal(rows, ref["rows"])


# 3. 64-bit sums, the grid stride, the edges ------------------------------------------
def test_sums_beyond_32_bits(renderer):
    """65536 x 1 x 1 samples under C4's plane: N = 65536, Q_00 about 9.4e13, by
    closed form and evaluated."""
    spec = ((-2.0, -0.5, 0.3), (6.1e-5, 0.01, 0.01), (65536, 1, 1), 0.0)
    f = frame_of("C4")
    ref = reference("wide", "C4", spec)
    rows, counts = run(renderer, f, spec)
    dense, dcounts = run(renderer, f, spec, dense=True)
    print(f"wide: row 0 {rows[0].tolist()} counts {counts} dense {dcounts}")
    assert ref["rows"][0, 0] == 65536 and ref["rows"][0, 4] == 65535 * 65536 * 131071 // 6
    assert np.array_equal(rows, ref["rows"][:1]) and np.array_equal(dense, ref["rows"][:1])
    assert counts[2] == dcounts[2] == 8192 and dcounts[0] == 8192 and counts[1] > 0


def test_more_bricks_than_workgroups(renderer):
    """C1's sphere through a column of MEASURE_MAX_BLOCKS + 5 bricks: a workgroup
    takes several bricks."""
    k = abi.MEASURE_MAX_BLOCKS
    spec = ((-0.15, 0.25, -0.2), (0.1, 0.15, 0.39 / (8 * (k + 5))), (3, 2, 8 * (k + 5)), 0.0)
    ref = reference("stride", "C1", spec)
    rows, counts = run(renderer, frame_of("C1"), spec)
    print(f"stride: row 0 {rows[0].tolist()} counts {counts}")
    assert 0 < ref["rows"][0, 0] < 3 * 2 * 8 * (k + 5)
    assert counts[2] == k + 5 and np.array_equal(rows, ref["rows"][:1])


@pytest.mark.parametrize("name,spec", [
    ("one-inside", ((-0.02, 0.38, -0.02), (0.04, 0.04, 0.04), (1, 1, 1), 0.0)),
    ("one-outside", ((0.5, 0.9, 0.5), (0.04, 0.04, 0.04), (1, 1, 1), 0.0)),
    ("brick", ((-0.21, 0.19, -0.2), (0.05, 0.05, 0.05), (8, 8, 8), 0.0)),
    ("nine", ((-0.23, 0.39, -0.01), (0.05, 0.05, 0.05), (9, 1, 1), 0.0)),
    ("empty", ((2.0, 2.0, 2.0), (0.05, 0.05, 0.05), (9, 8, 17), 0.0)),
])
@pytest.mark.parametrize("flags", [0, OWN], ids=["all", "owners"])
def test_edges(renderer, name, spec, flags):
    ref = reference(("edge", name), "C1", spec)
    rows, counts = run(renderer, frame_of("C1"), spec, flags)
    assert np.array_equal(rows, want_rows(ref, flags)), name
    assert counts[2] == ref["bricks"][2]
    n = ref["rows"][0, 0]
    assert n == {"one-inside": 1, "one-outside": 0, "empty": 0}.get(name, n)
    if n == 0:
        assert rows[0, 10:13].tolist() == list(spec[2]) and rows[0, 13:16].tolist() == [-1, -1, -1]


def test_a_stale_workspace_changes_nothing(renderer):
    for flags in (0, OWN):
        rows, counts, _, _, _ = exact_run(renderer, "C4", flags)
        kind, *spec = CASES["C4"]
        got, c = run(renderer, frame_of(kind), spec, flags, fill=0xFF)
        assert np.array_equal(got, rows) and c == counts


# 4. fast precision --------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FAST_CASES))
def test_fast_rows_equal_the_reference(renderer, case):
    """No sample is within FAST_BOUND_T of a change of sign, so no inside bit can
    differ: row 0 equals the reference exactly; the owner rows add up to it, and
    equal the reference where no owner decision is closer than the bound.
    Integers cannot show that the fast unit ran: the run-time specialised
    C4-carved holds that by its compilation count."""
    kind, *spec = FAST_CASES[case]
    f = frame_of(kind, FAST)
    ref = reference(("fast", case), kind, spec)
    assert ref["min_abs_w"] > FP.FAST_BOUND_T
    got = {}
    for flags in (0, OWN):
        first = FP.first_use(("measure", flags, kind)) if kind in FP.JIT else None
        n0 = renderer.lib.sdf_jit_count()
        got[flags], _ = run(renderer, f, spec, flags)
        n1 = renderer.lib.sdf_jit_count()
        again, _ = run(renderer, f, spec, flags)
        assert np.array_equal(got[flags], again)
        if first is not None:
            assert (n1 - n0, renderer.lib.sdf_jit_count() - n1) == (first, 0)
    rows = got[OWN]
    print(f"{case}: min |w| {ref['min_abs_w']:.3e} owner gap {ref['min_owner_gap']:.3e} "
          f"row 0 {rows[0].tolist()}")
    assert np.array_equal(got[0], ref["rows"][:1]) and np.array_equal(rows[:1], ref["rows"][:1])
    assert np.array_equal(rows[1:, :10].sum(axis=0), rows[0, :10])
    assert np.array_equal(rows[1:, 10:13].min(axis=0), rows[0, 10:13])
    assert np.array_equal(rows[1:, 13:16].max(axis=0), rows[0, 13:16])
    if ref["min_owner_gap"] > FP.FAST_BOUND_T:
        assert np.array_equal(rows, ref["rows"])


# 5. the public layers -------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def test_renderer_measure_is_the_abi_call(renderer):
    kind, origin, cell, n, iso = FAST_CASES["C1"]
    f = frame_of(kind)
    ref = reference("public", kind, (origin, cell, n, iso))
    g = R.grid(origin, cell, n)
    want = MS.Measure(ref["rows"], (0, 0, ref["bricks"][2], 0), tuple(g.origin), tuple(g.cell), n)
    m = renderer.measure(f, origin, cell, n, iso, owners=True)
    assert np.array_equal(m.rows, ref["rows"]) and m.counts[2:] == (ref["bricks"][2], 0)
    assert m.volume() == want.volume() > 0 and _same(m.centroid(), want.centroid())
    assert _same(m.covariance(), want.covariance()) and _same(m.inertia(2.5), want.inertia(2.5))
    assert _same(m.bounds(), want.bounds()) and m.mass([3.0]) == want.mass([3.0]) == 3.0 * m.volume()
    plain = renderer.measure(f, origin, cell, n, iso, dense=True)
    assert np.array_equal(plain.rows, ref["rows"][:1]) and plain.counts[0] == plain.counts[2]


def test_cpp_host_program_measure(renderer, tmp_path):
    """sdf_main --measure prints what Renderer.measure's helpers give for its csg8
    scene (C3's) on that box, with and without densities: the same fp64 bits
    (sdf::Measure evaluates in measure.py's order, and %.17g round-trips).  When
    nothing weighs anything, centroid and inertia are null and the line is still
    JSON."""
    f = frame_of("C3")
    box = "-1.25,-0.125,-1,1.25,1.125,1,20"
    spec = ((-1.25, -0.125, -1.0), (0.125, 0.0625, 0.1), 20)
    rho = [0.0, 1.0, 2.0, 0.5, 1.0, 1.0, 3.0, 1.0]
    for dens in (None, rho, [0.0] * 8):
        extra = ["--density", ",".join(str(d) for d in dens)] if dens else []
        r = sdf_main("--measure", box, *extra, "64", "36", "1", tmp_path / "f.ppm", "csg8")
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"measure"')]
        assert len(line) == 1, r.stdout
        got = json.loads(line[0], parse_constant=lambda name: pytest.fail(f"{name} is no JSON"))
        got = got["measure"]
        m = renderer.measure(f, *spec, owners=dens is not None)
        assert got["volume"] == m.volume() > 0
        assert got["mass"] == (m.mass(dens) if dens else m.volume())
        if dens is not None and not any(dens):
            assert got["mass"] == 0.0 and got["centroid"] is None and got["inertia"] is None
        else:
            assert _same(got["centroid"], m.centroid(dens))
            assert _same(got["inertia"], m.inertia(1.0, dens))
        assert _same(got["bounds"], m.bounds())
        assert (got["bricks"]["evaluated"], got["bricks"]["closed_form"], got["bricks"]["all"]) == \
            m.counts[:3]
