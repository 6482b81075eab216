"""The reference of mirror reflections (tests/reflect_ref.c / reflect_ref.py)
checked against itself and against the references it builds on, without a GPU:
what the GPU tests compare the kernels with must itself be the contract of
include/sdf_abi.h "Reflections", and must not hold vacuously."""
import functools

import numpy as np
import pytest

import lights_ref as LR
import materials_ref as MR
import oracle
import reflect_ref as RR
from sdf3d_amd import abi, scenes

f32 = np.float32
PRIM_FRAMES = MR.FRAMES
ALL_FRAMES = MR.FRAMES + [("C5", 0)]


def frame_of(name, pose):
    if name in ("C5", "C1"):
        return scenes.config(name, *RR.SHAPE, precision=abi.PRECISION_EXACT, pose=pose)
    return MR.frame_of(name, pose)


def mats_of(f):
    return MR.palette_for(f) if f.scene.kind == abi.SCENE_PRIMITIVES else [f.material]


@functools.lru_cache(maxsize=None)
def ref(name, pose, bounces, strength=1.0):
    f = frame_of(name, pose)
    return (f,) + RR.render(f, mats_of(f), bounces, strength)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.mark.parametrize("name,pose", PRIM_FRAMES)
def test_no_bounce_is_the_materials_reference(name, pose):
    f, rgba, steps, w = ref(name, pose, 0)
    mats = mats_of(f)
    fold = MR.fold(f, mats)
    for k in ("amb", "dif", "ref", "P"):
        assert np.array_equal(bits(w[k][:, :, 0]), bits(fold[k])), k
    terms = oracle.render_terms(f)
    want = MR.compose_px(f, [terms], [f.light], fold["amb"], fold["dif"], fold["ref"])
    assert np.array_equal(bits(rgba), bits(want))
    _, osteps = oracle.render(f)
    assert np.array_equal(steps, osteps)
    assert w["alive"].all()


def test_no_bounce_on_the_mandelbulb_is_the_oracle():
    f, rgba, steps, _ = ref("C5", 0, 0)
    want, osteps = oracle.render(f)
    assert np.array_equal(bits(rgba), bits(want)) and np.array_equal(steps, osteps)


@pytest.mark.parametrize("name,pose", ALL_FRAMES)
def test_strength_zero_is_no_bounce(name, pose):
    _, r0, s0, _ = ref(name, pose, 0)
    _, r3, s3, w = ref(name, pose, 3, 0.0)
    assert np.array_equal(bits(r3), bits(r0)) and np.array_equal(s3, s0)
    assert not w["alive"][:, :, 1:].any()


@pytest.mark.parametrize("name,pose", ALL_FRAMES)
@pytest.mark.parametrize("bounces", [1, 3])
def test_planes_are_finite_and_the_composite_is_their_fold(name, pose, bounces):
    f, rgba, steps, w = ref(name, pose, bounces)
    for k in ("O", "D", "P", "N", "d", "ao", "amb", "dif", "ref", "W", "C", "difs", "xs"):
        assert np.isfinite(w[k]).all(), k
    assert np.isfinite(rgba).all()
    # the weights the C walk carried are the NumPy statement's
    assert np.array_equal(bits(w["W"]), bits(RR.weights(w["ref"], w["alive"], 1.0)))
    # the composite, written out once more channel by channel
    acc = w["C"][:, :, 0].copy()
    for j in range(1, bounces + 1):
        add = (acc + (w["W"][:, :, j] * w["C"][:, :, j]).astype(f32)).astype(f32)
        acc = np.where(w["alive"][:, :, j, None], add, acc)
    assert np.array_equal(bits(rgba[..., :3]), bits(acc)) and (rgba[..., 3] == 1).all()
    assert np.array_equal(steps[..., 0], w["sp"].sum(axis=2))
    assert np.array_equal(steps[..., 1], w["ss"].sum(axis=(2, 3)))
    # one plain light: a layer's colour is the oracle's own shade_pixel's
    assert np.array_equal(bits(w["own"][w["alive"]]), bits(w["C"][w["alive"]]))
    # a layer of a shorter path is the same layer of a longer one
    _, _, _, w1 = ref(name, pose, 1)
    assert np.array_equal(bits(w1["C"]), bits(w["C"][:, :, :2]))


@pytest.mark.parametrize("name,pose", ALL_FRAMES)
def test_a_path_ends_on_a_miss_and_on_a_matte_surface(name, pose):
    f, _, _, w = ref(name, pose, 3)
    alive, d = w["alive"], w["d"]
    assert alive[:, :, 0].all()
    for j in range(3):
        nxt = alive[:, :, j + 1]
        assert not (nxt & ~alive[:, :, j]).any()
        assert not (nxt & (d[:, :, j] > f.params.max_dist)).any(), "a path went on past a miss"
        k = (f32(1.0) * w["ref"][:, :, j]).astype(f32)
        wn = (w["W"][:, :, j] * k).astype(f32)
        goes = alive[:, :, j] & ~(d[:, :, j] > f.params.max_dist) & ~(wn == 0).all(axis=-1)
        assert np.array_equal(nxt, goes)
    # a matte table reflects nothing
    mats = mats_of(f)
    matte = [type(m).from_buffer_copy(m) for m in mats]
    for m in matte:
        m.ref[0] = m.ref[1] = m.ref[2] = 0.0
    r0, s0, _ = RR.render(f, matte, 0, 1.0)
    r2, s2, w2 = RR.render(f, matte, 2, 1.0)
    assert np.array_equal(bits(r2), bits(r0)) and np.array_equal(s2, s0)
    assert not w2["alive"][:, :, 1:].any()


def test_the_ground_plane_mirrors_y():
    f, _, _, w = ref("REF", 0, 1)
    N, D, D1 = w["N"][:, :, 0], w["D"][:, :, 0], w["D"][:, :, 1]
    plane = w["alive"][:, :, 1] & (N[..., 0] == 0) & (N[..., 1] == 1) & (N[..., 2] == 0)
    assert plane.mean() > 0.2, "REF's plane fills a good part of the frame"
    # exactly, as values (N's zeros may carry either sign, and with them R's)
    want = D * np.array([1, -1, 1], dtype=f32)
    assert np.array_equal(D1[plane], want[plane])
    # the next eye is the shadow march's origin: P lifted by offset * eps along N
    p = f.params
    oy = (w["P"][:, :, 0, 1] + f32(1.0) * f32(p.shadow_offset) * f32(p.eps)).astype(f32)
    assert np.array_equal(bits(w["O"][:, :, 1, 1][plane]), bits(oy[plane]))


@pytest.mark.parametrize("name,pose,least", [(n, p, 0.10) for n, p in PRIM_FRAMES] + [("C5", 0, 0.05)])
def test_reflections_are_there_to_be_checked(name, pose, least):
    """What keeps the GPU tests from passing vacuously: with strength 1 and the
    palette a good share of the pixels see something in their first bounce, and
    the composite differs visibly from the frame without bounces."""
    f, rgba, _, w = ref(name, pose, 1)
    hit = w["alive"][:, :, 1] & (w["d"][:, :, 1] <= f.params.max_dist)
    assert hit.mean() >= least, hit.mean()
    _, r0, _, _ = ref(name, pose, 0)
    assert np.abs(rgba[..., :3] - r0[..., :3]).max() >= 0.1


def test_several_lights_and_forced_steps():
    f = frame_of("C4", 0)
    mats = mats_of(f)
    lights = LR.rig(3)
    rgba, steps, w = RR.render(f, mats, 2, 1.0, lights, abi.LIGHTS_COLOR)
    assert np.isfinite(rgba).all() and w["ss"].shape[-1] == 3
    # layer 0 is the materials reference under the same lights
    fold = MR.fold(f, mats)
    terms = [oracle.render_terms(LR.with_light(f, l)) for l in lights]
    want = MR.compose_px(f, terms, lights, fold["amb"], fold["dif"], fold["ref"],
                         flags=abi.LIGHTS_COLOR)
    assert np.array_equal(bits(w["C"][:, :, 0]), bits(want[..., :3]))
    # a replay at the walk's own counts is the walk
    force = np.zeros(w["alive"].shape + (RR.FORCE,), dtype=np.int32)
    force[..., 0] = w["sp"]
    force[..., 1:4] = w["ss"]
    again, steps2, w2 = RR.render(f, mats, 2, 1.0, lights, abi.LIGHTS_COLOR, force=force)
    assert np.array_equal(bits(again), bits(rgba)) and np.array_equal(steps2, steps)
    # one step fewer on layer 1's primary march moves its hit point
    force[:, :, 1, 0] = np.maximum(w["sp"][:, :, 1] - 1, 0)
    _, _, w3 = RR.render(f, mats, 2, 1.0, lights, abi.LIGHTS_COLOR, force=force)
    moved = w["alive"][:, :, 1] & (w["sp"][:, :, 1] > 1)
    assert (w3["P"][:, :, 1][moved] != w["P"][:, :, 1][moved]).any()
    assert np.array_equal(bits(w3["C"][:, :, 0]), bits(w["C"][:, :, 0]))
