"""CPU checks of the queries' reference (tests/query_ref.py) against the
oracle itself, and of the input conditions the GPU tests rely on."""
import numpy as np
import pytest

import materials_ref as MR
import oracle
import query_ref as Q
from sdf3d_amd import abi, scenes

f32 = np.float32


def frame(name, w=64, h=36):
    return scenes.config(name, w, h)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture(scope="module")
def rays():
    o, d = Q.ray_set()
    return o, Q.normalize(d)


def test_normalize_is_the_oracles():
    """|D| of the set's directions within an ulp of 1, and the three-division
    form (not a reciprocal)."""
    _, d = Q.ray_set()
    D = Q.normalize(d)
    x, y, z = (d[:, i] for i in range(3))
    l = np.sqrt((x * x + y * y) + z * z)
    assert np.array_equal(bits(D[:, 1]), bits(y / l))
    assert np.all(np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1) < 2e-7)


@pytest.mark.parametrize("name", ["REF", "C1", "C4", "C5"])
def test_replay_at_own_steps_is_the_march(name, rays):
    """The forced-step replay at the oracle's own step counts reproduces
    oracle.raymarch, bits and steps."""
    f = frame(name)
    O, D = rays
    t, st = Q.march(f, O, D)
    r = Q.replay(f, O, D, st)
    assert np.array_equal(bits(r), bits(t))
    assert st.min() >= 1 and st.max() <= f.params.max_steps


@pytest.mark.parametrize("name", ["REF", "C4"])
def test_camera_rays_give_the_renders_steps(name):
    """The restated camera rays, marched by oracle.raymarch, give exactly
    oracle.render's primary step counts at 37 x 23."""
    f = frame(name, 37, 23)
    _, steps = oracle.render(f)
    O, D = Q.camera_rays(f)
    _, st = Q.march(f, O, D)
    assert np.array_equal(st.reshape(23, 37), steps[..., 0])


def test_owner_on_the_reference_scene(rays):
    """REF: the floor is primitive 0, the sphere primitive 1."""
    f = frame("REF")
    O, D = rays
    h = Q.hits(f, O, D)
    hit = h["hit"]
    assert hit.sum() > 50 and (~hit).sum() > 10
    # the marches that converged (the others ran out of steps grazing the floor)
    on = hit & (h["steps"] < f.params.max_steps)
    P = h["P"][on]
    sphere = np.linalg.norm(P.astype(np.float64) - [0.0, 0.4, 0.0], axis=1) < 0.2 + 0.02
    floor = np.abs(P[:, 1]) < 0.02
    assert np.all(sphere ^ floor) and sphere.sum() >= 5
    assert np.array_equal(h["prim"][on], sphere.astype(np.int32))
    assert np.all(h["prim"][~hit] == -1) and not h["normal"][~hit].any()
    # and directly: points on each surface
    w, _ = Q.owner(f, np.array([[1.0, 0.0, 1.0], [0.0, 0.6, 0.0], [0.2, 0.4, 0.0]], dtype=f32))
    assert list(w) == [0, 1, 1]


def test_owner_names_every_primitive_of_csg8():
    """A point on each primitive of C4, away from the blends, is owned by it."""
    f = frame("C4")
    P = np.array([[2.0, 0.0, 2.0], [0.0, 0.6, 0.0], [-0.7, 0.3, -0.3], [0.9, 0.16, -0.3],
                  [0.05, 0.52, 0.3], [0.45, 0.5, 0.35], [-0.4, 0.24, -0.8], [0.25, 0.67, -0.15]],
                 dtype=f32)
    w, gap = Q.owner(f, P)
    assert list(w) == list(range(8))
    assert np.all(np.abs(Q.scene_sdf(f, P)) < 0.02)


@pytest.mark.parametrize("name", ["REF", "C4", "C5"])
def test_ray_set_conditions(name, rays):
    """Input condition of the fast-precision GPU test (materials_ref.GAP, the
    materials tests' own rule): at most 2 % of the hit rays have an owner
    decision closer than GAP; and the set exercises every branch on C4."""
    f = frame(name)
    O, D = rays
    h = Q.hits(f, O, D)
    hit = h["hit"]
    close = hit & (h["min_gap"] < MR.GAP)
    print(f"{name}: {hit.sum()} of {len(O)} rays hit, {close.sum()} close owner decisions, "
          f"{(h['steps'] == f.params.max_steps).sum()} marches out of steps, "
          f"{(h['steps'] == 1).sum()} ending at step 1")
    assert close.sum() <= 0.02 * hit.sum()
    if name == "C4":
        assert hit.sum() >= 100 and (~hit).sum() >= 20
        assert (h["steps"] == f.params.max_steps).sum() >= 1
        assert len(set(h["prim"][hit])) >= 4


def test_hand_rays_in_the_oracle():
    """What the oracle makes of the hand-made rays on C4: the zero direction
    normalises to NaN and marches to max_steps with a NaN distance (C4's first
    smooth union turns the NaN point into a NaN distance); the ray from inside
    the sphere, the scaled ones and the grazing one are ordinary rays."""
    f = frame("C4")
    O, d = Q.hand_rays()
    h = Q.trace(f, O, d)
    z = Q.ZERO_DIR
    assert np.isnan(h["t"][z]) and h["steps"][z] == f.params.max_steps and h["hit"][z]
    assert np.isnan(h["normal"][z]).all() and h["prim"][z] == 0
    rest = np.arange(len(O)) != z
    assert np.isfinite(h["t"][rest]).all()
    assert Q.scene_sdf(f, O[1:2])[0] < 0          # inside a primitive
    # scaling a direction does not change its ray
    a = Q.trace(f, O[2:4], d[2:4])
    b = Q.trace(f, O[2:4], (d[2:4] * f32([[1e3], [1e-3]])).astype(f32))
    assert np.array_equal(a["steps"], b["steps"])
    assert np.allclose(a["t"], b["t"], rtol=1e-5)
