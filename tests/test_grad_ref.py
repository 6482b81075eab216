"""CPU tests that tie tests/grad_ref.py (the reference of sdf_sample_grad) to the
project: its forward value against the CPU oracle, its autograd against its own
finite differences, the smooth-min partials sdf_abi.h "Gradients" states in
closed form, and the implicit-function formula of autograd.trace on a sphere.
"""
import numpy as np
import pytest
import torch

import grad_ref
import oracle
from sdf3d_amd import abi

FRAMES = grad_ref.all_frames()
POINTS = grad_ref.cube_points(200)


@pytest.mark.parametrize("name", list(FRAMES))
def test_forward_matches_oracle(name):
    """fp64 reference against the fp32 oracle: 1e-5 max(1, |f|) -- fp32 epsilon
    times a few tens of operations at coordinates <= 10."""
    f = FRAMES[name]
    ref = grad_ref.gradients(f.scene, POINTS).f.numpy()
    want = np.array([oracle.scene_sdf(f.scene, float(x), float(y), float(z)) for x, y, z in POINTS])
    assert np.all(np.abs(ref - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("name", list(FRAMES))
def test_kink_exclusions_stay_rare(name):
    """The GPU tests leave out points whose kink margin is below 1e-4 max(1, |p|):
    at most 5 % of a scene's points, by the reference alone."""
    f = FRAMES[name]
    r = grad_ref.gradients(f.scene, POINTS)
    keep = grad_ref.kink_mask(r.margin.numpy(), POINTS)
    assert (~keep).mean() <= 0.05, (~keep).sum()


def _value(kinds, ops, theta, pts):
    return grad_ref.scene_value(kinds, ops, theta, pts)[0]


@pytest.mark.parametrize("name", ["C4", "jit4"] + [grad_ref.coverage_frame(k, o).name
                                                     for k, o in grad_ref.COVERAGE])
def test_autograd_matches_finite_differences(name):
    """The reference's autograd against its own fp64 central differences (h =
    1e-5) for every parameter slot and the points, on the points with kink margin
    >= 1e-3; 1e-6 relative to max(1, |value|): two orders above truncation plus
    rounding at that h."""
    f = FRAMES[name]
    h = 1e-5
    r = grad_ref.gradients(f.scene, POINTS)
    keep = torch.from_numpy(r.margin.numpy() >= 1e-3)
    assert keep.sum() >= 100
    kinds, ops, theta = grad_ref.scene_lists(f.scene)
    theta = theta.to(torch.float32).to(torch.float64)
    pts = torch.from_numpy(POINTS).to(torch.float64)[keep]
    rk = grad_ref.gradients(f.scene, POINTS[keep.numpy()])
    # parameters: d/dtheta sum_i f_i
    for i in range(len(kinds)):
        for s in [2] + list(range(4, 11)):
            if s == 2 and ops[i] not in grad_ref.SMOOTH:
                continue   # a hard operator has no k (and k = 0 cannot be stepped below 0)
            lo, hi = theta.clone(), theta.clone()
            lo[i, s] -= h
            hi[i, s] += h
            fd = ((_value(kinds, ops, hi, pts) - _value(kinds, ops, lo, pts)) / (2 * h)).sum()
            got = rk.grad_prims[i, s]
            assert abs(got - fd) <= 1e-6 * max(1.0, abs(float(fd))), (i, s, float(got), float(fd))
    # points: df_i/dp_i
    for c in range(3):
        lo, hi = pts.clone(), pts.clone()
        lo[:, c] -= h
        hi[:, c] += h
        fd = (_value(kinds, ops, theta, hi) - _value(kinds, ops, theta, lo)) / (2 * h)
        got = rk.grad_points[:, c]
        assert torch.all((got - fd).abs() <= 1e-6 * torch.clamp(fd.abs(), min=1.0))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_smooth_partials_closed_form(sign):
    """m_a = (b < a) ? h/2 : 1 - h/2, m_b = 1 - m_a, m_k = h h / 4 - h / 2."""
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(4096, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    b = (a.detach() + sign * torch.rand(4096, generator=g, dtype=torch.float64) * 0.5).requires_grad_()
    k = (0.05 + torch.rand(4096, generator=g, dtype=torch.float64) * 0.6).requires_grad_()
    ev = grad_ref._Eval(4096, torch.float64)
    m = ev.smin(a, b, k)
    ga, gb, gk = torch.autograd.grad(m.sum(), (a, b, k))
    h = torch.clamp(k - (a - b).abs(), min=0.0) / k
    h = h.detach()
    ma = torch.where(b < a, h / 2, 1 - h / 2)
    assert (h > 0).any() and (h == 0).any()
    assert torch.allclose(ga, ma, rtol=0, atol=1e-14)
    assert torch.allclose(gb, 1 - ma, rtol=0, atol=1e-14)
    assert torch.allclose(gk, h * h / 4 - h / 2, rtol=0, atol=1e-14)


def test_implicit_trace_formula_on_a_sphere():
    """t(theta, O, D) of a ray and a sphere is closed-form; its derivatives must
    equal dt/dtheta = -(df/dtheta)(P) / (G . D), dt/dO = -G / (G . D), dt/dD = t
    dt/dO with G = grad f(P), P = O + t D."""
    from sdf3d_amd import scenes
    f = scenes.config("C1", 64, 36)
    base = grad_ref.scene_lists(f.scene)[2]      # the scene's fp32 values, exactly
    c = base[0, 4:7].clone().requires_grad_()
    r = base[0, 7].clone().requires_grad_()
    rng = np.random.default_rng(3)
    for _ in range(8):
        o = torch.tensor(rng.uniform(-1, 1, 3) + [0, 0.4, 2.0], dtype=torch.float64,
                         requires_grad=True)
        aim = torch.tensor([0.0, 0.4, 0.0]) + torch.tensor(rng.uniform(-0.1, 0.1, 3))
        d0 = (aim - o.detach())
        d = (d0 / d0.norm()).to(torch.float64).requires_grad_()
        oc = o - c
        qa, qb, qc = d.dot(d), oc.dot(d), oc.dot(oc) - r * r
        t = (-qb - torch.sqrt(qb * qb - qa * qc)) / qa
        gc, gr, go, gd = torch.autograd.grad(t, (c, r, o, d))
        P = (o + t * d).detach().numpy()[None, :]
        # the formula is exact at the exact P: evaluate the reference there in fp64
        # (grad_ref rounds points to fp32, so pass the scene's function directly)
        kinds, ops, theta = grad_ref.scene_lists(f.scene)
        th = theta.clone().requires_grad_()
        pp = torch.from_numpy(P).requires_grad_()
        val, _ = grad_ref.scene_value(kinds, ops, th, pp)
        G, gth = torch.autograd.grad(val.sum(), (pp, th))
        G = G[0]
        gdot = G.dot(d.detach())
        assert abs(float(val.detach())) < 1e-12
        assert torch.allclose(-G / gdot, go, rtol=1e-9, atol=1e-12)
        assert torch.allclose(float(t.detach()) * -G / gdot, gd, rtol=1e-9, atol=1e-12)
        assert torch.allclose(-gth[0, 4:7] / gdot, gc, rtol=1e-9, atol=1e-12)
        assert torch.allclose(-gth[0, 7] / gdot, gr, rtol=1e-9, atol=1e-12)


def test_fit_reference_converges():
    """The step count and rate were chosen so that the fp64 reference drives the
    loss below 0.1 % of its start; the GPU test must then reach 1 %."""
    from sdf3d_amd import autograd
    tgt, start = grad_ref.fit_frames()
    pts = grad_ref.fit_points(tgt).to(torch.float64)
    kinds, ops, _ = grad_ref.scene_lists(tgt.scene)
    th0 = autograd.scene_tensor(start.scene).to(torch.float64)
    first, last, _ = grad_ref.fit(lambda th: grad_ref.scene_value(kinds, ops, th, pts)[0], th0)
    assert last <= 1e-3 * first, (first, last)
