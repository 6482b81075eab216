"""CPU checks of the fast-precision launch-path tests (tests/fast_paths.py):
that each comparison fails when fed another kernel's results -- the oracle's
results for plain C4 judged as C4-carved's -- and gives exactly 0 on the
reference's own; that the shares the GPU tests may leave out are met by the
reference alone; and that the oracle's new probes agree with the old ones."""
import numpy as np
import pytest

import fast_paths as FP
import materials_ref as MR
import mesh_ref as M
import oracle
import query_ref as Q
from cases import C4_GRID
from cases import query_frame as frame_of
from fast_paths import FAST_BOUND_N, FAST_BOUND_T, MESH_BOUND_N
from fast_paths import MESH_BOUND_V as FAST_BOUND_V
from gpu_support import ndiff
from sdf3d_amd import abi, scenes

f32 = np.float32


def carved():
    return FP.PATHS["C4-carved"]()


@pytest.fixture(scope="module")
def rays():
    return Q.ray_set()


@pytest.fixture(scope="module")
def traced(rays):
    """The oracle's sdf_trace of the 200-ray set on plain C4 and on C4-carved."""
    return {k: Q.trace(f, *rays) for k, f in (("C4", frame_of("C4")), ("carved", carved()))}


@pytest.fixture(scope="module")
def sampled():
    """The oracle's sdf_sample of the grid on plain C4 and on C4-carved."""
    P = Q.grid()
    return {k: (Q.scene_sdf(f, P), Q.normals(f, P))
            for k, f in (("C4", frame_of("C4")), ("carved", carved()))}


@pytest.fixture(scope="module")
def meshed():
    """The reference meshes of plain C4 and of C4-carved on C4_GRID."""
    return {k: M.mesh(f, *C4_GRID) for k, f in (("C4", frame_of("C4")), ("carved", carved()))}


def test_carved_has_no_built_in_signature_but_c4s_kinds():
    a, b = frame_of("C4").scene, carved().scene
    assert a.count == b.count == 8
    assert [p.kind for p in a.prims[:8]] == [p.kind for p in b.prims[:8]]
    differ = [i for i in range(8) if a.prims[i].op != b.prims[i].op]
    assert differ == [FP.CARVED] and b.prims[FP.CARVED].op == abi.OP_SMOOTH_SUBTRACT
    assert a.prims[FP.CARVED].kind == abi.PRIM_ROUND_BOX
    assert carved().params.dispatch == abi.DISPATCH_AUTO


# ---- 1. a plain C4 kernel would be caught ------------------------------------------

def test_plain_c4_rays_violate_the_bound(rays, traced):
    r = Q.fast_deviation(carved(), *rays, traced["C4"], MR.GAP)
    print(f"plain C4's rays judged as C4-carved's: {r}")
    assert r["t"] > FAST_BOUND_T
    assert r["steps_differ"] >= 10


def test_plain_c4_points_violate_the_bound(sampled):
    r = FP.point_deviation(carved(), Q.grid(), *sampled["C4"])
    beyond = int((np.abs(sampled["C4"][0].astype(np.float64) - sampled["carved"][0])
                  > FAST_BOUND_T).sum())
    print(f"plain C4's points judged as C4-carved's: {r}; {beyond} points beyond the bound")
    assert r["dist"] > FAST_BOUND_T and r["normal"] > FAST_BOUND_N
    assert beyond >= 100


def test_plain_c4_mesh_has_another_connectivity(meshed):
    r = M.fast_deviation(meshed["carved"], meshed["C4"], C4_GRID[1])
    print(f"plain C4's mesh {meshed['C4']['counts']} judged as C4-carved's "
          f"{meshed['carved']['counts']}: {r}")
    assert not r["same_connectivity"]
    assert not (r["vertex_over_cell"] <= FAST_BOUND_V) and not (r["normal"] <= MESH_BOUND_N)


# ---- 2. the reference's own results deviate by exactly 0 ---------------------------

def test_exact_results_pass_every_check(rays, traced, sampled, meshed):
    """Which is why the GPU tests also assert that the fast output differs from
    the exact one in some bit."""
    r = Q.fast_deviation(carved(), *rays, traced["carved"], MR.GAP)
    assert r["t"] == 0 and r["normal"] == 0 and r["prim_wrong"] == 0 and r["steps_differ"] == 0
    assert r["normal_rays"] == r["hit"]
    p = FP.point_deviation(carved(), Q.grid(), *sampled["carved"])
    assert p["dist"] == 0 and p["normal"] == 0
    m = M.fast_deviation(meshed["carved"], meshed["carved"], C4_GRID[1])
    assert m["same_connectivity"] and m["vertex_over_cell"] == 0 and m["normal"] == 0
    assert m["prim_wrong"] == 0
    assert ndiff(sampled["carved"][0], sampled["carved"][0]) == 0
    assert ndiff(sampled["carved"][0], sampled["C4"][0]) > 0


def test_point_deviation_counts_nonfinite_values():
    f, P = frame_of("REF"), Q.grid()[:8]
    dist, nrm = Q.scene_sdf(f, P), Q.normals(f, P)
    bad = dist.copy()
    bad[3] = np.nan
    assert FP.point_deviation(f, P, bad, nrm)["dist"] == np.inf
    bad = nrm.copy()
    bad[5, 1] = np.nan
    assert FP.point_deviation(f, P, dist, bad)["normal"] == np.inf


# ---- 3. the shares left out, by the reference alone ----------------------------------

@pytest.mark.parametrize("kind", ["REF", "C4", "C4-generic", "C4-unculled", "C4-carved", "C5"])
def test_points_left_out_are_few(kind):
    f, P = frame_of(kind), Q.grid()
    r = FP.point_deviation(f, P, Q.scene_sdf(f, P), Q.normals(f, P))
    ref = FP.point_reference(f, P)
    spread = float(np.nanmax(np.abs(ref["fma"].astype(np.float64) - ref["normal"])))
    print(f"{kind}: {r['normal_left_out']} of {r['points']} points left out; the contracted "
          f"reading's normals differ by up to {spread:.3e}")
    assert r["points"] == 17 * 13 * 11
    assert r["normal_left_out"] <= FP.LEFT_OUT_SHARE * r["points"]


def test_carved_ray_set_and_lattice_conditions(traced, meshed):
    h = traced["carved"]
    close = h["hit"] & (h["min_gap"] < MR.GAP)
    print(f"C4-carved: {int(h['hit'].sum())} rays hit, {int(close.sum())} close owner decisions; "
          f"lattice min |w| {meshed['carved']['min_abs_w']:.3e}, counts {meshed['carved']['counts']}")
    assert h["hit"].sum() >= 100
    assert close.sum() <= FP.LEFT_OUT_SHARE * h["hit"].sum()
    assert meshed["carved"]["min_abs_w"] >= 1e-4
    assert meshed["carved"]["counts"] != meshed["C4"]["counts"]


# ---- 4. the oracle's new probes ------------------------------------------------------

def test_the_f64_probes_round_to_the_fp32_ones():
    """On REF's grid the twin's distance is the fp32 oracle's within 1e-6.  Its
    normal cannot be that close: the fp32 normal is a difference of fp32 taps
    2 h = 0.02 apart, so half an ulp of a tap near 1 (6e-8) already moves a
    component by 3e-6 (5.64e-6 is the largest here).  It is held to
    FAST_BOUND_N / 4 instead, the threshold beyond which point_deviation leaves
    a point out: on REF the twin leaves none out."""
    f, P = frame_of("REF"), Q.grid()
    d32 = Q.scene_sdf(f, P)
    d64 = np.array([oracle.scene_sdf(f.scene, *map(float, p), reading="f64") for p in P])
    n32 = Q.normals(f, P)
    n64 = np.stack([oracle.normal(f.scene, f.params, p, reading="f64") for p in P])
    assert d64.dtype == n64.dtype == np.float64
    print(f"REF: twin against fp32 oracle: dist {np.abs(d64 - d32).max():.3e} "
          f"normal {np.abs(n64 - n32).max():.3e}")
    assert np.abs(d64 - d32).max() <= 1e-6
    assert np.abs(n64 - n32).max() <= FAST_BOUND_N / 4
    assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() <= 1e-12
    assert (d64 != d32).any()                     # and it is not the fp32 value widened


def test_the_fma_reading_is_the_contracted_library():
    f, P = frame_of("C4"), Q.grid()[::7]
    lib = oracle.load("fma")
    import ctypes as C
    out = (C.c_float * 3)()
    for p in P:
        x, y, z = map(float, p)
        want = f32(lib.sdf_oracle_scene_sdf(C.byref(f.scene), x, y, z))
        got = f32(oracle.scene_sdf(f.scene, x, y, z, reading="fma"))
        assert Q.bits_of(got) == Q.bits_of(want)
        lib.sdf_oracle_normal(C.byref(f.scene), C.byref(f.params), (C.c_float * 3)(x, y, z), out)
        n = oracle.normal(f.scene, f.params, p, reading="fma")
        assert np.array_equal(Q.bits_of(n), Q.bits_of(np.array(list(out), dtype=f32)))
    with pytest.raises(KeyError):
        oracle.scene_sdf(f.scene, 0.0, 0.0, 0.0, reading="other")
