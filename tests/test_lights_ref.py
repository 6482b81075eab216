"""CPU tests of the multi-light reference (tests/lights_ref.py): for one plain
light it is the oracle's colour bit for bit, its single-rounded fma agrees
with exact rational arithmetic, and the rig lights the test frames usefully
(asserted on the oracle alone)."""
import random
from fractions import Fraction

import numpy as np
import pytest

import lights_ref as LR
import oracle
from sdf3d_amd import abi, scenes

f32 = np.float32
_TERMS = {}


def frame_of(cfg, pose, prec=abi.PRECISION_EXACT):
    return scenes.config(cfg, *LR.SHAPE, precision=prec, pose=pose)


def oracle_terms(cfg, pose, i):
    """The oracle's terms of (cfg, pose) under rig light i alone: computed
    once, shared, read-only."""
    key = (cfg, pose, i)
    if key not in _TERMS:
        t = oracle.render_terms(LR.with_light(frame_of(cfg, pose), LR.rig(8)[i]))
        t.setflags(write=False)
        _TERMS[key] = t
    return _TERMS[key]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("cfg,pose", LR.FRAMES)
def test_one_plain_light_is_the_oracle_render(cfg, pose):
    f = frame_of(cfg, pose)
    for light in (f.light, LR.rig(2)[1]):
        g = LR.with_light(f, light)
        ref, _ = oracle.render(g)
        out = LR.compose(g, [oracle.render_terms(g)], [light], 0, abi.PRECISION_EXACT)
        assert same(out, ref)


def round_fraction(v: Fraction) -> np.float32:
    """v rounded to float32, to nearest and ties to even, by exact comparison
    with the neighbouring floats."""
    x = f32(float(v))
    if not np.isfinite(x):
        return x
    cands = {float(x), float(np.nextafter(x, f32(-np.inf))), float(np.nextafter(x, f32(np.inf)))}
    cands = [c for c in cands if np.isfinite(c)]
    best = min(abs(Fraction(c) - v) for c in cands)
    near = [c for c in cands if abs(Fraction(c) - v) == best]
    if len(near) > 1:
        near = [c for c in near if (int(f32(c).view(np.uint32)) & 1) == 0]
    assert len(near) == 1
    return f32(near[0])


def fma_triples(n=10000, seed=20260419):
    rng = random.Random(seed)
    out = []
    # constructed midpoints: (1 + 2^-j)^2 = 1 + 2^(1-j) + 2^-2j lies exactly
    # between two floats for j = 12, and a c far below fp64's ulp decides the
    # side -- a multiply-add rounded in fp64 first loses it
    for j in (12,):
        for e in (-60, -70, -100, -149):
            for sign in (1.0, -1.0):
                for scale in (1.0, 2.0 ** 10, 2.0 ** -20, -1.0):
                    a = (1.0 + 2.0 ** -j) * scale
                    out.append((a, 1.0 + 2.0 ** -j, sign * 2.0 ** e * abs(scale)))
    # a product that is a midpoint with c = 0 (a tie, to even) and with c one
    # ulp of fp32 either way
    out += [(1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, 0.0),
            (1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, 2.0 ** -23),
            (3.0 * (1.0 + 2.0 ** -12), 1.0 + 2.0 ** -12, -2.0 ** -22)]
    # cancellation, subnormal results, and values as the colour sum has them
    while len(out) < n:
        kind = rng.randrange(4)
        if kind == 0:
            a, b, c = (rng.uniform(-2, 2) for _ in range(3))
        elif kind == 1:
            a, b = rng.uniform(0, 1), rng.uniform(0, 1)
            c = -float(f32(f32(a) * f32(b))) + rng.choice([0.0, 2.0 ** -30, -2.0 ** -40])
        elif kind == 2:
            a, b, c = rng.uniform(0, 1) * 2.0 ** -70, rng.uniform(0, 1) * 2.0 ** -70, \
                rng.uniform(-1, 1) * 2.0 ** -140
        else:
            a = float(np.ldexp(rng.uniform(1, 2), rng.randrange(-30, 30)))
            b = float(np.ldexp(rng.uniform(1, 2), rng.randrange(-30, 30)))
            c = float(np.ldexp(rng.uniform(-2, 2), rng.randrange(-60, 60)))
        out.append((a, b, c))
    return np.asarray(out[:n], dtype=f32)


def test_fma_is_rounded_once():
    t = fma_triples()
    assert len(t) == 10000
    got = LR.fma32(t[:, 0], t[:, 1], t[:, 2])
    want = np.asarray([round_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
                       for a, b, c in t], dtype=f32)
    assert same(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    # the constructed cases do tell the two apart: fp64 multiply-add rounded
    # twice misses some of them
    twice = (t[:, 0].astype(np.float64) * t[:, 1].astype(np.float64)
             + t[:, 2].astype(np.float64)).astype(f32)
    assert not same(twice[:40], want[:40])


@pytest.mark.parametrize("cfg,pose", LR.FRAMES)
def test_rig_lights_the_frames(cfg, pose):
    terms = [oracle_terms(cfg, pose, i) for i in range(8)]
    for t in terms:
        assert np.isfinite(t).all()
        # the geometry does not depend on the light
        assert same(t[..., 0], terms[0][..., 0])
    if cfg == "C1":
        return      # kept as an edge case: the sphere alone fills 4 % of the frame
    lit = (terms[0][..., 1] > 0) & (terms[1][..., 1] > 0)
    assert lit.mean() >= 0.20, lit.mean()


@pytest.mark.parametrize("cfg,pose", LR.FRAMES)
def test_primary_steps_do_not_depend_on_the_light(cfg, pose):
    f = frame_of(cfg, pose)
    steps = [oracle.render(LR.with_light(f, l))[1] for l in LR.rig(3)]
    for s in steps[1:]:
        assert np.array_equal(s[..., 0], steps[0][..., 0])


def test_order_and_flag_matter():
    """The contract pins the lights' order and the colour flag: the rig's
    frames change bits when either does."""
    f = frame_of("C4", 0)
    lights = LR.rig(3)
    terms = [oracle_terms("C4", 0, i) for i in range(3)]
    a = LR.compose(f, terms, lights, 0)
    b = LR.compose(f, terms[::-1], lights[::-1], 0)
    c = LR.compose(f, terms, lights, abi.LIGHTS_COLOR)
    assert not same(a, b) and not same(a, c)
    assert np.allclose(a, b, rtol=0, atol=1e-5)
