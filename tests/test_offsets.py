"""Culling on unit-size scenes far from the origin (no GPU): the host-side
bounds of sdf_scene_bounds on scenes moved by tests/offsets.py, without being
scaled, to coordinates of 1e3 ... 2^20.

  containment   every bound, as the kernel reads it (fp32 centre, K'), holds
                its primitive's true sphere, with no tolerance
  fresh test    the kernels' culling test, restated in NumPy fp32, against the
                oracle at adversarial points: on and just outside the bounding
                shell, where the bound is tight, with a competitor whose value
                sweeps across the primitive's.  Wherever the test says "far",
                the primitive must not change the oracle's value by a bit
  range         beyond the coordinate magnitude the margins are proven for, the
                plan does not cull

The parent of the commit that added this file (a capsule's bound around its
unrounded midpoint, the radius not knowing of the rounding) fails the
containment at every moved offset (all 48 cases), the capsule fresh test at
11 of the 24 cases from 1e4 on -- hard union at 1e4-skew, both operators at
1e5 and 2^20 -- and has no range beyond which it stops culling
(profiles/cull_offsets.json)."""
import ctypes as C

import numpy as np
import pytest

import offsets as O
import oracle
from bounds_ref import check_containment
from cases import random_scene
from sdf3d_amd import abi, scenes

NAMES = list(O.OFFSETS)


def template():
    return scenes.config("C3", 64, 64).scene


# ---- the helper itself ----------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C4", "C5", "REF"])
def test_zero_offset_is_the_frame_itself(cfg):
    f = scenes.config(cfg, 96, 54, pose=1)
    g = O.translate(f, O.OFFSETS["0"])
    for a, b in ((f.scene, g.scene), (f.camera, g.camera), (f.light, g.light),
                 (f.material, g.material), (f.params, g.params)):
        assert O.same_bytes(a, b)


@pytest.mark.parametrize("name", O.MOVED)
def test_translation_moves_everything_and_scales_nothing(name):
    """The oracle's own camera position moves by T (to the fp32 spacing at T),
    its ray directions are unchanged, the plane still passes through the moved
    origin, sizes and blend radii keep their bits."""
    T = O.OFFSETS[name]
    f = scenes.config("C4", 96, 54, pose=2)
    g = O.translate(f, T)
    u0, u1 = oracle.uniforms(f.camera, f.params), oracle.uniforms(g.camera, g.params)
    ulp = np.spacing(np.float32(np.abs(T).max())).astype(np.float64)
    assert np.all(np.abs(u1["cam"].astype(np.float64) - (u0["cam"] + T)) <= 4 * ulp)
    assert np.array_equal(u0["inv_view"][:12], u1["inv_view"][:12])
    assert u0["focal"] == u1["focal"] and O.same_bytes(f.params, g.params)
    for i in range(f.scene.count):
        a, b = f.scene.prims[i], g.scene.prims[i]
        assert (a.kind, a.op, a.k) == (b.kind, b.op, b.k)
        if a.kind == abi.PRIM_PLANE:
            assert list(a.p[0:3]) == list(b.p[0:3])
            n = np.array(a.p[0:3], dtype=np.float64)
            assert abs(n @ T + b.p[3] - a.p[3]) <= ulp
            continue
        moved = 6 if a.kind == abi.PRIM_CAPSULE else 3
        assert np.all(np.abs(np.array(b.p[:moved], dtype=np.float64) -
                             (np.array(a.p[:moved]) + np.tile(T, moved // 3))) <= ulp)
        assert list(a.p[moved:]) == list(b.p[moved:])
    assert np.all(np.abs(np.array(g.light.pos, dtype=np.float64) -
                         (np.array(f.light.pos) + T)) <= ulp)


# ---- containment ------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("name", NAMES)
def test_translated_scenes_are_contained(name, seed):
    """Random scenes of every kind (cases.random_scene) moved by T: every
    primitive's true sphere, float64 from its fp32 parameters, lies inside the
    sphere the kernel reads, |c_f - c_true| + R_true <= K'(1 - kCullRel) -
    kCullAbs - k, and the cullable ones inside the cluster sphere -- with no
    tolerance at all (bounds_ref.check_containment)."""
    rng = np.random.default_rng(7000 + seed)
    while True:     # a draw that ends in a hard-union sphere culls little: one with a subject
        scene = random_scene(rng, abi.SDF_MAX_PRIMS)
        if O.bounds_of(scene)[3] <= abi.SDF_MAX_PRIMS - 8:
            break
    assert check_containment(O.translate_scene(scene, O.OFFSETS[name])) is not None


@pytest.mark.parametrize("name", NAMES)
def test_translated_capsules_are_contained(name):
    """The same on capsules alone, whose centre is the one the host computes
    (a midpoint, which rounds) instead of a parameter: 15 per scene."""
    rng = np.random.default_rng(7100)
    for _ in range(6):
        s = template()
        C.memset(C.addressof(s.prims), 0, C.sizeof(s.prims))
        s.count = abi.SDF_MAX_PRIMS
        s.prims[0].kind, s.prims[0].op = abi.PRIM_PLANE, abi.OP_UNION
        s.prims[0].p[1] = 1.0
        for i in range(1, s.count):
            op = abi.OP_SMOOTH_UNION if i % 2 else abi.OP_UNION
            O.random_primitive(rng, abi.PRIM_CAPSULE, op, s.prims[i])
        assert check_containment(O.translate_scene(s, O.OFFSETS[name])) is not None


# ---- the fresh test against the oracle ----------------------------------------------
MIN_SUBJECT = 100


def fresh_case(kind, op, name, min_subject=MIN_SUBJECT, max_scenes=40):
    """Scenes [competitor, primitive] of (kind, op) at offset `name`, until at
    least `min_subject` probe points inside the sweep lie on either side of the
    restated test.  Returns dict of the counts: points, far and near (both
    inside the sweep), far_all, and violations: far points at which the pair's
    value is not the competitor's, bit for bit."""
    rng = np.random.default_rng(4321 + 16 * kind + op)
    tmpl = template()
    r = {"scenes": 0, "points": 0, "far": 0, "near": 0, "far_all": 0, "violations": 0}
    while r["scenes"] < max_scenes and min(r["far"], r["near"]) < min_subject:
        s, P = O.pair_scene(tmpl, O.OFFSETS[name], rng, kind, op)
        is_far, d = O.says_far(s, 1, P)
        win = O.in_sweep(s, 1, P, d)
        pair = O.sdf_at(s, P)
        r["scenes"] += 1
        r["points"] += len(P)
        r["far"] += int((is_far & win).sum())
        r["near"] += int((~is_far & win).sum())
        r["far_all"] += int(is_far.sum())
        r["violations"] += int((is_far & (pair.view(np.uint32) != d.view(np.uint32))).sum())
    return r


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind,op", O.CULLABLE,
                         ids=[f"{abi.PRIM_NAMES[k]}-{abi.OP_NAMES[o]}" for k, o in O.CULLABLE])
def test_far_points_leave_the_oracle_value_unchanged(kind, op, name):
    """Wherever the restated test calls a probe point far, oracle.scene_sdf of
    [competitor, primitive] equals oracle.scene_sdf of the competitor alone,
    bit for bit.  The points lie beyond the primitive's farthest features, up to
    1 away, in the cone where a competitor sphere's value d sweeps across the
    primitive's s: d - s (hard union) or d + k - s (smooth union) over +-2e-3.
    The test has a subject: at least 100 far points and at least 100 near
    points inside that sweep, and below 2^20 at least 100 far points inside the
    sweep as well.  At 2^20 most far points lie outside it -- the recorded
    capsule smooth-union case at 2^20-skew has 41 inside -- so the adversarial
    part of the subject is thinner there: a capsule's bound then carries its
    midpoint's rounding, up to 0.11, more than the sweep is wide."""
    r = fresh_case(kind, op, name)
    print(f"{abi.PRIM_NAMES[kind]} {abi.OP_NAMES[op]} at {name}: {r}")
    assert r["violations"] == 0
    assert r["far_all"] >= MIN_SUBJECT and r["near"] >= MIN_SUBJECT
    if O.magnitude(name) < 2.0 ** 20:
        assert r["far"] >= MIN_SUBJECT


# ---- the proven range -----------------------------------------------------------------
CULL_MAX_COORD = 2.0 ** 22      # sdf_abi.cpp kCullMaxCoord


@pytest.mark.parametrize("axis", range(3))
def test_no_culling_beyond_the_proven_range(axis):
    """The margins are an argument for cullable primitives that reach no
    further than 2^22 from the origin (|c|_inf + R + k, DESIGN.md "Culling
    margins at large coordinates"); beyond it sdf_scene_bounds reports
    cluster_first = count: nothing is culled.  C4 moved along one axis, just
    inside and just outside.  sdf_scene_bounds takes no params and reports the
    generic kernel's bounds; a render plan stops earlier, at |c|_inf + R + k +
    max_dist > 2^22, so within max_dist below 2^22 sdf_scene_bounds still
    reports a cluster while no plan culls (include/sdf_abi.h says so; on the
    GPU tests/test_gpu_offsets.py holds a frame beyond the range)."""
    f = scenes.config("C4", 64, 64)
    _, _, _, first = O.bounds_of(f.scene)
    assert first == 1
    for sign in (1.0, -1.0):
        T = np.zeros(3)
        T[axis] = sign * (CULL_MAX_COORD - 4.0)
        rc, _, _, first = O.bounds_of(O.translate_scene(f.scene, T))
        assert (rc, first) == (0, 1), (axis, sign)
        T[axis] = sign * (CULL_MAX_COORD + 4.0)
        rc, b, cl, first = O.bounds_of(O.translate_scene(f.scene, T))
        assert (rc, first) == (0, f.scene.count), (axis, sign)


# ---- the fixed kernel's probe, by the bounds its plan reads ---------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("which", list(O.CSG8_PROBED))
def test_fixed_kernel_probe_is_far_by_the_plans_bounds(which, name):
    """The CSG8-signature probe of tests/test_gpu_offsets.py, by the oracle and
    the restated test alone.  The fixed kernel's plan caches gaps, so its bounds
    carry kCullPath (|c|_inf + R + k + max_dist) beside sdf_scene_bounds' -- 0.01
    at 1e4 and 1.0 at 2^20, far more than the sweep of +-2e-3 -- and the probe
    lowers its plane by up to 1.5 times that.  By a bracket of the plan's
    bounds (offsets.plan_bound) at least 100 points are far and 100 are not,
    and at every far point the scene with the probed primitive equals the scene
    cut before it, bit for bit."""
    rng = np.random.default_rng(977 + O.CSG8_PROBED[which])
    tmpl = scenes.config("C4", 64, 64).scene
    reach = float(scenes.config("C3", 64, 64).params.max_dist)
    far = points = violations = 0
    for _ in range(40):
        s, P, i = O.csg8_probe(tmpl, O.OFFSETS[name], rng, which, reach=reach)
        is_far, d = O.says_far(s, i, P, reach=reach)
        with_it = O.sdf_at(O.cut(s, i + 1), P)
        violations += int((is_far & (with_it.view(np.uint32) != d.view(np.uint32))).sum())
        far += int(is_far.sum())
        points += len(P)
        if far >= MIN_SUBJECT and points - far >= MIN_SUBJECT:
            break
    print(f"CSG8 {which} at {name}: {points} points, {far} far by the plan's bounds, "
          f"{violations} violations")
    assert violations == 0
    assert far >= MIN_SUBJECT and points - far >= MIN_SUBJECT
