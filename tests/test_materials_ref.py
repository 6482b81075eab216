"""CPU tests of the material fold's reference (tests/materials_ref.c over the
CPU oracle; include/sdf_abi.h "Materials"): known answers of the fold, and the
condition on the inputs that the GPU tests of fast precision rely on -- few
pixels whose hard owner decision is closer than materials_ref.GAP."""
import ctypes as C

import numpy as np
import pytest

import lights_ref as LR
import materials_ref as MR
import oracle
from sdf3d_amd import abi, scenes

f32 = np.float32
_FOLD = {}


def fold(name, pose):
    if (name, pose) not in _FOLD:
        f = MR.frame_of(name, pose)
        r = MR.fold(f, MR.palette_for(f))
        for v in r.values():
            v.setflags(write=False)
        _FOLD[(name, pose)] = (f, r)
    return _FOLD[(name, pose)]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.mark.parametrize("name,pose", [("REF", 0), ("C4", 0), ("SIX", 2), ("SIXH", 2)])
def test_uniform_materials_fold_to_that_material(name, pose):
    f = MR.frame_of(name, pose)
    m = scenes.palette(5)[4]
    r = MR.fold(f, [m] * f.scene.count)
    for got, want in zip((r["amb"], r["dif"], r["ref"]), MR.constant(f, m)):
        assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name,pose", MR.FRAMES)
def test_final_distance_is_the_scene_sdf(name, pose):
    f, r = fold(name, pose)
    P, d = r["P"], r["d"]
    assert np.isfinite(P).all()
    want = np.array([[oracle.scene_sdf(f.scene, *map(float, P[y, x])) for x in range(P.shape[1])]
                     for y in range(P.shape[0])], dtype=f32)
    assert np.array_equal(bits(d), bits(want))


def test_point_is_the_oracles_hit_point():
    """P of a hit pixel lies on the surface the oracle's colour shows: the fold
    runs at the oracle's own P, whose scene distance is below eps on a hit."""
    f, r = fold("REF", 0)
    _, steps = oracle.render(f)
    hit = steps[..., 0] < f.params.max_steps
    assert hit.any() and (np.abs(r["d"][hit & (r["d"] < 1.0)]) < 0.05).all()


def test_reference_scene_owner_is_sphere_or_plane():
    f, r = fold("REF", 0)
    P = r["P"].astype(f32)
    plane = P[..., 1]                                        # planeSDF: p.y
    c = np.array([0.0, 0.4, 0.0], dtype=f32)
    q = P - c
    sphere = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2])
                     .astype(f32)).astype(f32) - f32(0.2)
    want = (sphere < plane).astype(int)                      # a tie keeps the plane
    assert np.array_equal(r["owner"], want)
    assert 0 < want.sum() < want.size and not r["blended"].any()
    pal = MR.palette_for(f)
    for i in (0, 1):
        sel = r["owner"] == i
        assert np.array_equal(bits(r["dif"][sel]), bits(np.broadcast_to(
            np.array(list(pal[i].dif), dtype=f32), r["dif"][sel].shape)))


def two_spheres(op, k):
    f = scenes.config("C3", *MR.SHAPE)
    C.memset(C.addressof(f.scene.prims), 0, C.sizeof(f.scene.prims))
    f.scene.count = 2
    scenes._prim(f.scene, 0, abi.PRIM_SPHERE, abi.OP_UNION, 0.0, -0.25, 0.5, 0.0, 0.3)
    scenes._prim(f.scene, 1, abi.PRIM_SPHERE, op, k, 0.25, 0.5, 0.0, 0.3)
    return f


def test_equal_spheres_blend_half_on_the_symmetry_plane():
    f = two_spheres(abi.OP_SMOOTH_UNION, 0.1)
    a, b = abi.sdf_material(), abi.sdf_material()
    for c in range(3):
        a.amb[c] = a.dif[c] = a.ref[c] = 0.0
        b.amb[c], b.dif[c], b.ref[c] = 1.0, 2.0, -4.0
    for y, z in ((0.5, 0.0), (0.7, 0.1), (0.3, -0.2), (5.0, 3.0)):
        m, d, gap, owner, blended, t = MR.fold_at(f.scene, [a, b], 0.0, y, z)
        assert t == f32(0.5) and blended
        assert list(m) == [0.5] * 3 + [1.0] * 3 + [-2.0] * 3
        assert bits(d) == bits(f32(oracle.scene_sdf(f.scene, 0.0, y, z)))
    # far on either side the nearer sphere owns the point outright
    m, _, _, owner, blended, t = MR.fold_at(f.scene, [a, b], -0.6, 0.5, 0.0)
    assert (t, owner, blended) == (0.0, 0, False) and list(m) == [0.0] * 9
    m, _, _, owner, blended, t = MR.fold_at(f.scene, [a, b], 0.6, 0.5, 0.0)
    assert (t, owner, blended) == (1.0, 1, False) and list(m[3:6]) == [2.0] * 3


def test_hard_operators_own_what_they_carve():
    a, b = scenes.palette(2)
    # subtraction: inside the cutter's reach the cutter owns the carved surface
    f = two_spheres(abi.OP_SUBTRACT, 0.0)
    _, d, gap, owner, _, t = MR.fold_at(f.scene, [a, b], -0.05, 0.5, 0.0)   # on the cut
    assert (t, owner) == (1.0, 1) and abs(d) < 1e-6
    _, _, _, owner, _, t = MR.fold_at(f.scene, [a, b], -0.55, 0.5, 0.0)     # far side of sphere 0
    assert (t, owner) == (0.0, 0)
    # intersection: the primitive whose surface bounds the lens there
    f = two_spheres(abi.OP_INTERSECT, 0.0)
    _, _, _, owner, _, t = MR.fold_at(f.scene, [a, b], 0.05, 0.5, 0.0)      # sphere 0's far cap
    assert (t, owner) == (0.0, 0)
    _, _, _, owner, _, t = MR.fold_at(f.scene, [a, b], -0.05, 0.5, 0.0)     # sphere 1's near cap
    assert (t, owner) == (1.0, 1)
    # a tie keeps the earlier owner
    f = two_spheres(abi.OP_UNION, 0.0)
    _, _, gap, owner, _, t = MR.fold_at(f.scene, [a, b], 0.0, 0.5, 0.0)
    assert (t, owner, gap) == (0.0, 0, 0.0)


def test_smooth_intersect_and_subtract_blend():
    a, b = scenes.palette(2)
    for op in (abi.OP_SMOOTH_INTERSECT, abi.OP_SMOOTH_SUBTRACT):
        # between the centres |a - b| is 0.04 (intersection) and 0.1
        # (subtraction): h = 0.87 and 0.67 with k = 0.3
        f = two_spheres(op, 0.3)
        x = 0.02
        m, d, _, _, blended, t = MR.fold_at(f.scene, [a, b], x, 0.5, 0.0)
        want = 0.376 if op == abi.OP_SMOOTH_INTERSECT else 0.778
        assert blended and abs(t - want) < 2e-3, t
        assert bits(d) == bits(f32(oracle.scene_sdf(f.scene, x, 0.5, 0.0)))
        lo, hi = np.minimum(list(a.dif), list(b.dif)), np.maximum(list(a.dif), list(b.dif))
        assert ((m[3:6] >= lo - 1e-6) & (m[3:6] <= hi + 1e-6)).all()


def test_six_variants_are_different_scenes_with_the_same_owners():
    """The two SIX frames show the same owner counts; they are nevertheless two
    scenes: where primitive 6 owns the pixel the final distances differ (a
    sphere's against a box's), and nowhere in these frames does primitive 6
    blend, so the counts agree for a reason."""
    (_, s), (_, h) = fold("SIX", 2), fold("SIXH", 2)
    assert np.array_equal(s["owner"], h["owner"])
    assert sorted(np.unique(s["owner"])) == list(range(7))
    six = s["owner"] == 6
    assert six.sum() > 100 and (bits(s["d"][six]) != bits(h["d"][six])).all()
    assert np.array_equal(s["blended"], h["blended"])
    assert np.array_equal(bits(s["dif"][~six]), bits(h["dif"][~six]))


def test_compose_px_with_constant_arrays_is_compose():
    f = MR.frame_of("C3", 2)
    lights = LR.rig(3)
    terms = [oracle.render_terms(LR.with_light(f, l)) for l in lights]
    amb, dif, ref = MR.constant(f, f.material)
    for flags in (0, abi.LIGHTS_COLOR):
        want = LR.compose(f, terms, lights, flags)
        got = MR.compose_px(f, terms, lights, amb, dif, ref, flags)
        assert np.array_equal(bits(got), bits(want))
    specs = [LR.spec_exact(t[..., 2], 12.0) for t in terms]
    want = LR.compose(f, terms, lights, abi.LIGHTS_COLOR, abi.PRECISION_FAST, specs=specs)
    got = MR.compose_px(f, terms, lights, amb, dif, ref, abi.LIGHTS_COLOR, abi.PRECISION_FAST,
                        specs=specs)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name,pose", MR.FRAMES)
def test_few_pixels_have_a_close_hard_decision(name, pose):
    """A condition on the inputs of the GPU tests: at most 2 % of a frame's
    pixels may have min_gap < GAP (they are left out of the comparison of fast
    precision with this reference)."""
    _, r = fold(name, pose)
    share = float((r["min_gap"] < MR.GAP).mean())
    print(f"{name}: min_gap < {MR.GAP}: {100 * share:.2f} % of the pixels, "
          f"blended {100 * float(r['blended'].mean()):.2f} %")
    assert share <= 0.02
