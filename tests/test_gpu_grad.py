"""GPU tests of sdf_sample_grad and sdf3d_amd/autograd.py (sdf_abi.h "Gradients")
against tests/grad_ref.py, the scene spec in torch float64 differentiated by
torch's CPU autograd.

Accuracy has no stored constant: E32 is the deviation of the SAME reference run
in float32 from the float64 one on the same inputs, and the kernel's deviation by
the same metric must stay within 4 x E32 in exact precision (a different but
equally valid fp32 order of the same operations) and 8 x E32 in fast precision
(1-ulp reciprocal, rsq and sqrt, contraction).
  grad_points: the largest |component error| / max(1, |g_i|).
  grad_prims:  the largest |error| / S over the slots, S = sum_i |g_i| |df_i/dtheta|
               in fp64, each slot's value floored at 2^-20.
Points whose kink margin is below 1e-4 max(1, |p|) may take another branch in
fp32: they are left out of the grad_points comparison and get upstream 0, in the
kernel's run and the reference's alike.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_ref
from gpu_support import PAD, fenced, untouched, with_precision
from sdf3d_amd import abi, scenes
from sdf3d_amd import autograd as ag

pytestmark = pytest.mark.gpu

FRAMES = grad_ref.all_frames()
POINTS = grad_ref.cube_points(200)
SENTINEL = 12345.0
FLOOR = grad_ref.FLOOR
BOUND = {abi.PRECISION_EXACT: 4.0, abi.PRECISION_FAST: 8.0}
PRECISIONS = [abi.PRECISION_EXACT, abi.PRECISION_FAST]
GRID_CAPACITY = 1024 * 256      # lanes of the capped grid


def raw_call(rd, frame, pts, upstream=None, dist=True, grad_points=True, grad_prims=True,
             workspace=True):
    """sdf_sample_grad on fenced buffers (PAD guard elements behind each, which
    must survive); every buffer starts filled with SENTINEL.  Returns
    (dist, grad_points, grad_prims) as CPU numpy arrays (None when not asked for)."""
    n = pts.shape[0]
    dev = rd.device

    def buf(want, m):
        return fenced(torch, dev, (m,), torch.float32, guard=PAD).fill_(SENTINEL) if want else None
    d, gp, gt = buf(dist, n), buf(grad_points, 3 * n), buf(grad_prims, 256)
    nbytes = int(rd.lib.sdf_grad_workspace_bytes(n)) if (grad_prims and workspace) else 0
    ws = buf(nbytes > 0, nbytes // 4)
    out = abi.sdf_grad_out(*[C.c_void_p(x.data_ptr()) if x is not None else None
                             for x in (d, gp, gt)])
    rc = rd.lib.sdf_sample_grad(
        C.byref(frame.scene), C.byref(frame.params), C.c_void_p(pts.data_ptr()), n,
        C.c_void_p(upstream.data_ptr()) if upstream is not None else None, C.byref(out),
        C.c_void_p(ws.data_ptr()) if ws is not None else None, nbytes,
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    abi.check(rc, "sdf_sample_grad")
    torch.cuda.synchronize()
    res = []
    for x in (d, gp, gt, ws):
        if x is None:
            res.append(None)
            continue
        assert untouched(torch, x), "a store went past the end of its buffer"
        res.append(x.cpu().numpy())
    if res[1] is not None:
        res[1] = res[1].reshape(n, 3)
    if res[2] is not None:
        res[2] = res[2].reshape(16, 16)
    return res[0], res[1], res[2]


_cases = {}


def case(name, n=200):
    key = (name, n)
    if key not in _cases:
        pts = POINTS if n == 200 else grad_ref.cube_points(n, seed=77 + n % 1000)
        _cases[key] = grad_ref.Case(FRAMES[name], pts)
    return _cases[key]


def run_case(rd, frame, c, **kw):
    pts = torch.from_numpy(c.points).to(rd.device)
    up = torch.from_numpy(c.upstream).to(rd.device)
    return raw_call(rd, frame, pts, up, **kw)


def check_accuracy(rd, name, n, prec):
    c = case(name, n)
    f = with_precision(FRAMES[name], prec)
    dist, gp, gt = run_case(rd, f, c)
    assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gt))
    assert np.all(gt[c.count:] == 0.0) and np.all(gt[:, [0, 1, 3]] == 0.0)
    if prec == abi.PRECISION_EXACT:
        want, _ = rd.sample(f, torch.from_numpy(c.points).to(rd.device))
        assert np.array_equal(dist.view(np.uint32), want.cpu().numpy().view(np.uint32))
    e_pts, e_prims = c.e32()
    k_pts, k_prims = c.points_error(gp), c.prims_error(gt)
    print(f"grad {name} n={n} prec={prec}: points {k_pts:.3e} / E32 {e_pts:.3e}, "
          f"prims {k_prims:.3e} / E32 {e_prims:.3e}")
    assert k_pts <= BOUND[prec] * e_pts
    assert k_prims <= BOUND[prec] * e_prims


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_gradients_match_reference(renderer, name, prec):
    check_accuracy(renderer, name, 200, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_counts(renderer, n, prec):
    check_accuracy(renderer, "C4", n, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_above_grid_capacity(renderer, prec):
    """grid x block + 7 points: the grid-stride loop runs twice for some lanes,
    every workspace row is used; accuracy, dist bits, sentinels and determinism."""
    n = GRID_CAPACITY + 7
    assert int(renderer.lib.sdf_grad_workspace_bytes(n)) == \
        int(renderer.lib.sdf_grad_workspace_bytes(1 << 30))
    check_accuracy(renderer, "C4", n, prec)
    c = case("C4", n)
    f = with_precision(FRAMES["C4"], prec)
    a = run_case(renderer, f, c, dist=False, grad_points=False)[2]
    b = run_case(renderer, f, c, dist=False, grad_points=False)[2]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["C4", "jit4", "capsule-ssub"])
def test_deterministic_and_null_forms(renderer, name, prec):
    rd = renderer
    c = case(name)
    f = with_precision(FRAMES[name], prec)
    d0, p0, t0 = run_case(rd, f, c)
    d1, p1, t1 = run_case(rd, f, c)
    for x, y in ((d0, d1), (p0, p1), (t0, t1)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # upstream NULL is an upstream of ones, bit for bit
    pts = torch.from_numpy(c.points).to(rd.device)
    ones = torch.ones(pts.shape[0], dtype=torch.float32, device=rd.device)
    _, pn, tn = raw_call(rd, f, pts, None)
    _, po, to = raw_call(rd, f, pts, ones)
    assert np.array_equal(pn.view(np.uint32), po.view(np.uint32))
    assert np.array_equal(tn.view(np.uint32), to.view(np.uint32))
    # without grad_prims no workspace is needed, and grad_points does not change
    _, pw, tw = run_case(rd, f, c, grad_prims=False, workspace=False)
    assert tw is None
    assert np.array_equal(pw.view(np.uint32), p0.view(np.uint32))
    # each output alone
    assert np.array_equal(run_case(rd, f, c, grad_points=False, grad_prims=False)[0].view(np.uint32),
                          d0.view(np.uint32))
    assert np.array_equal(run_case(rd, f, c, dist=False, grad_points=False)[2].view(np.uint32),
                          t0.view(np.uint32))
    # the wrapper is the same call
    up = torch.from_numpy(c.upstream).to(rd.device)
    g = rd.sample_grad(f, pts, up, dist=True)
    torch.cuda.synchronize()
    assert np.array_equal(g.dist.cpu().numpy().view(np.uint32), d0.view(np.uint32))
    assert np.array_equal(g.grad_points.cpu().numpy().view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(g.grad_prims.cpu().numpy().view(np.uint32), t0.view(np.uint32))


def test_mandelbulb_unsupported_and_no_jit(renderer):
    rd = renderer
    pts = torch.from_numpy(POINTS).to(rd.device)
    with pytest.raises(abi.SdfError) as e:
        rd.sample_grad(scenes.config("C5", 64, 36), pts, grad_prims=False)
    assert e.value.code == abi.SDF_E_UNSUPPORTED
    # a scene no built-in variant matches, under SDF_DISPATCH_AUTO: nothing is compiled
    f = FRAMES["jit6"].copy()
    f.params.dispatch = abi.DISPATCH_AUTO
    before = rd.lib.sdf_jit_count()
    rd.sample_grad(f, pts)
    torch.cuda.synchronize()
    assert rd.lib.sdf_jit_count() == before
    g = rd.sample_grad(f, pts[:0])
    assert g.grad_points.shape == (0, 3) and torch.all(g.grad_prims == 0)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_autograd_sample(renderer, prec):
    rd = renderer
    f = with_precision(FRAMES["C4"], prec)
    pts = torch.from_numpy(POINTS).to(rd.device)
    grads = {}
    for where in ("cpu", rd.device):
        theta = ag.scene_tensor(f.scene).to(where).requires_grad_()
        p = pts.clone().requires_grad_()
        dist = ag.sample(rd, f, theta, p)
        dist.square().mean().backward()
        assert theta.grad.device == theta.device and theta.grad.shape == theta.shape
        grads[str(where)] = (theta.grad.cpu(), p.grad.cpu(), dist.detach())
    a, b = grads["cpu"], grads[str(rd.device)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the corresponding upstream: d mean(f^2) / df_i = 2 f_i / n
    dist = a[2]
    up = (2.0 * dist / dist.shape[0]).contiguous()
    want = rd.sample_grad(f, pts, up, dist=True)
    assert torch.equal(want.dist, dist)
    assert torch.equal(want.grad_points.cpu(), a[1])
    assert torch.equal(want.grad_prims[: f.scene.count].cpu(), a[0])
    # only what requires a gradient is returned; n = 0 is handled in Python
    theta = ag.scene_tensor(f.scene).requires_grad_()
    ag.sample(rd, f, theta, pts).sum().backward()
    assert theta.grad is not None
    p = pts.clone().requires_grad_()
    ag.sample(rd, f, ag.scene_tensor(f.scene), p).sum().backward()
    assert p.grad is not None
    theta = ag.scene_tensor(f.scene).requires_grad_()
    ag.sample(rd, f, theta, pts[:0]).sum().backward()
    assert torch.all(theta.grad == 0)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_autograd_trace(renderer, prec):
    """d(sum t hit)/dtheta and d/dO on C4's 64 x 36 camera rays against the implicit
    formula evaluated with the fp64 reference at the kernel's own P.  The
    grad_prims metric and bound apply to theta (the terms are w_i df/dtheta(P_i), w_i
    = -1 / (G . D)), the grad_points metric to the origins (g_i = w_i).  Rays whose
    P sits on a kink, or within a factor 2 of the grazing threshold, are weighted
    out of the sum on both sides."""
    rd = renderer
    f = with_precision(scenes.config("C4", 64, 36), prec)
    n = 64 * 36
    o = torch.empty((n, 3), dtype=torch.float32, device=rd.device)
    d = torch.empty((n, 3), dtype=torch.float32, device=rd.device)
    abi.check(rd.lib.sdf_camera_rays(C.byref(f.camera), C.byref(f.params),
                                     C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream(rd.device).cuda_stream)))
    # the kernel's own t and P (the wrapper's forward, without autograd)
    unit = d / d.norm(dim=1, keepdim=True)
    t0 = rd.trace(f, o, unit.contiguous(), normal=False, prim=False, steps=False).t.cpu()
    found = ~(t0 > f.params.max_dist) & ~torch.isnan(t0)
    assert found.any() and (~found).any()          # hits and misses both occur
    D = unit.cpu().numpy().astype(np.float64)
    P = np.where(found.numpy()[:, None], (o.cpu() + t0[:, None] * unit.cpu()).numpy(),
                 o.cpu().numpy()).astype(np.float32)
    plain = grad_ref.gradients(f.scene, P)
    G = plain.grad_points.numpy()
    gd = (G * D).sum(axis=1)
    keep = found.numpy() & grad_ref.kink_mask(plain.margin.numpy(), P) & \
        (np.abs(gd) >= 2e-3 * np.linalg.norm(G, axis=1)) & (gd != 0)
    assert keep.sum() > 0.8 * found.sum().item()
    # the whole formula in fp64, and in fp32 (E32): G, then w = -1 / (G . D), then the sums
    w = np.where(keep, -1.0 / np.where(keep, gd, 1.0), 0.0)
    r64 = grad_ref.gradients(f.scene, P, w, torch.float64, round_upstream=False)
    G32 = grad_ref.gradients(f.scene, P, None, torch.float32).grad_points.numpy()
    gd32 = (G32 * D.astype(np.float32)).sum(axis=1)
    w32 = np.where(keep, -1.0 / np.where(keep, gd32, 1.0), 0.0).astype(np.float32)
    r32 = grad_ref.gradients(f.scene, P, w32, torch.float32)
    # the wrapper, differentiated: sum over the kept rays of t hit
    theta = ag.scene_tensor(f.scene).requires_grad_()
    oo = o.clone().requires_grad_()
    dd = d.clone().requires_grad_()
    t, hit = ag.trace(rd, f, theta, oo, dd)
    assert torch.equal(t.detach().cpu(), t0) and not hit.requires_grad
    sel = torch.from_numpy(keep).to(rd.device)
    (t * hit * sel).sum().backward()
    hit = hit.cpu().numpy()
    assert hit[keep].all() and not hit[~found.numpy()].any()
    # misses and grazing rays carry no gradient; nothing is NaN or INF
    g_o, g_d = oo.grad.cpu().numpy(), dd.grad.cpu().numpy()
    assert np.all(g_o[~keep] == 0) and np.all(g_d[~keep] == 0)
    assert np.all(np.isfinite(g_o)) and np.all(np.isfinite(g_d))
    assert torch.all(torch.isfinite(theta.grad))
    scale = r64.scale.numpy()
    live = scale > 0

    def prims_err(x):
        rel = np.abs(np.asarray(x, dtype=np.float64) - r64.grad_prims.numpy())[live] / scale[live]
        return float(np.maximum(rel, FLOOR).max())
    den = np.maximum(1.0, np.abs(w))[keep, None]

    def points_err(x):
        return float((np.abs(np.asarray(x, dtype=np.float64)[keep]
                             - r64.grad_points.numpy()[keep]) / den).max())
    k_prims, e_prims = prims_err(theta.grad.numpy()), prims_err(r32.grad_prims.numpy())
    k_pts, e_pts = points_err(g_o), points_err(r32.grad_points.numpy())
    print(f"trace prec={prec}: theta {k_prims:.3e} / E32 {e_prims:.3e}, "
          f"origins {k_pts:.3e} / E32 {e_pts:.3e}")
    assert k_prims <= BOUND[prec] * e_prims
    assert k_pts <= BOUND[prec] * e_pts


# ---- a fit (grad_ref.fit_*: the scene, the points, Adam's steps and rate) -----
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fit(renderer, prec):
    rd = renderer
    tgt, start = grad_ref.fit_frames()
    start = with_precision(start, prec)
    pts = grad_ref.fit_points(tgt).to(rd.device)
    first, last, theta = grad_ref.fit(lambda th: ag.sample(rd, start, th, pts),
                             ag.scene_tensor(start.scene))
    print(f"fit prec={prec}: loss {first:.3e} -> {last:.3e}")
    assert last <= 1e-2 * first
    want = ag.scene_tensor(tgt.scene)
    assert torch.all((theta - want).abs() <= 1e-2), (theta - want).abs().max()
