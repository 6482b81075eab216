"""torch.autograd over ``sdf_sample_grad`` (sdf_abi.h "Gradients").

The scene's float parameters travel as a tensor ``theta`` of shape (count, 16):
row i holds the sixteen 4-byte slots of ``sdf_primitive`` i as floats -- slot 0
the kind and slot 1 the operator (their integer values, never differentiated),
slot 2 the blend radius k, slot 3 reserved, slots 4 .. 15 the parameters p[0..11].

    theta = scene_tensor(frame.scene).requires_grad_()
    loss = sample(renderer, frame, theta, points).square().mean()
    loss.backward()          # theta.grad[i, 2], theta.grad[i, 4 + j]

All arithmetic runs in the HIP kernels; torch only carries the tensors.  Every
call copies ``theta`` to the host (about 1 KB) to fill the ``sdf_scene`` the
kernels read from their arguments: keep ``theta`` on the CPU, where that copy is
free -- a ``theta`` on the GPU costs a device-to-host synchronisation per call.
Gradients come back on ``theta``'s device either way.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi
from .renderer import Renderer
from .scenes import Frame

SLOTS = 16   # 4-byte slots of sdf_primitive


def _prims_view(scene: abi.sdf_scene, dtype) -> np.ndarray:
    """The scene's primitives as a (SDF_MAX_PRIMS, 16) array over its own memory."""
    buf = (C.c_char * C.sizeof(scene.prims)).from_address(C.addressof(scene.prims))
    return np.frombuffer(buf, dtype=dtype).reshape(abi.SDF_MAX_PRIMS, SLOTS)


def scene_tensor(scene: abi.sdf_scene) -> torch.Tensor:
    """(count, 16) float32 on the CPU: the primitives' slots as floats; the kind
    and op slots hold the integer values as floats."""
    n = int(scene.count)
    out = _prims_view(scene, np.float32)[:n].copy()
    out[:, 0:2] = _prims_view(scene, np.int32)[:n, 0:2]
    return torch.from_numpy(out)


def apply(scene: abi.sdf_scene, theta) -> abi.sdf_scene:
    """A copy of `scene` whose float slots (2 .. 15 of each primitive < count) are
    taken from `theta` (count, 16); kinds and operators stay the scene's."""
    n = int(scene.count)
    t = theta.detach().to("cpu", torch.float32).contiguous().numpy()
    if t.shape != (n, SLOTS):
        raise ValueError(f"theta must have shape ({n}, {SLOTS}), got {tuple(t.shape)}")
    out = abi.sdf_scene()
    C.memmove(C.addressof(out), C.addressof(scene), C.sizeof(scene))
    _prims_view(out, np.float32)[:n, 2:] = t[:, 2:]
    return out


def _frame_with(frame: Frame, theta) -> Frame:
    f = frame.copy()
    f.scene = apply(frame.scene, theta)
    return f


def _theta_grad(grad_prims, theta):
    return grad_prims[: theta.shape[0]].to(theta.device)


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, points, renderer, frame):
        f = _frame_with(frame, theta)
        pts = points.detach().contiguous()
        ctx.renderer, ctx.frame = renderer, f
        ctx.save_for_backward(theta, pts)
        if pts.shape[0] == 0:
            return pts.new_empty((0,))
        return renderer.sample_grad(f, pts, dist=True, grad_points=False, grad_prims=False).dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        theta, pts = ctx.saved_tensors
        want_theta, want_points = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_theta or want_points):
            return None, None, None, None
        if pts.shape[0] == 0:
            return (torch.zeros_like(theta) if want_theta else None,
                    torch.zeros_like(pts) if want_points else None, None, None)
        out = ctx.renderer.sample_grad(ctx.frame, pts, upstream=g.contiguous(), dist=False,
                                       grad_points=want_points, grad_prims=want_theta)
        return (_theta_grad(out.grad_prims, theta) if want_theta else None, out.grad_points,
                None, None)


def sample(renderer: Renderer, frame: Frame, theta, points) -> torch.Tensor:
    """The scene distance f(points; theta) (n,), differentiable once with respect
    to `theta` (count, 16; any device) and `points` (contiguous float32 (n, 3) on
    the renderer's device).  The scene is ``apply(frame.scene, theta)``; precision
    and the other parameters are the frame's.  Backward is one sdf_sample_grad
    call with the incoming gradient as upstream."""
    return _Sample.apply(theta, points, renderer, frame)


class _Trace(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, origins, unit_dirs, renderer, frame, min_cos):
        f = _frame_with(frame, theta)
        o, d = origins.detach().contiguous(), unit_dirs.detach().contiguous()
        n = o.shape[0]
        ctx.renderer, ctx.frame = renderer, f
        if n == 0:
            ctx.save_for_backward(theta, o, o.new_empty((0,)), o.new_empty((0,)))
            return o.new_empty((0,)), torch.zeros((0,), dtype=torch.bool, device=o.device)
        t = renderer.trace(f, o, d, normal=False, prim=False, steps=False).t
        found = ~(t > f.params.max_dist) & ~torch.isnan(t)
        # a finite point for every ray: the origin where nothing was found
        p = torch.where(found[:, None], o + t[:, None] * d, o).contiguous()
        grad = renderer.sample_grad(f, p, grad_prims=False).grad_points
        gd = (grad * d).sum(dim=1)
        hit = found & (gd != 0) & ~(gd.abs() < min_cos * grad.norm(dim=1))
        # dt/df at P by the implicit-function theorem: -1 / (G . D), 0 without a hit
        w = torch.where(hit, -1.0 / torch.where(hit, gd, torch.ones_like(gd)),
                        torch.zeros_like(gd))
        ctx.save_for_backward(theta, p, w, torch.where(hit, t, torch.zeros_like(t)))
        ctx.mark_non_differentiable(hit)
        return t, hit

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_t, _g_hit):
        theta, p, w, t = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return (None,) * 6
        if p.shape[0] == 0:
            return (torch.zeros_like(theta) if need[0] else None,
                    torch.zeros_like(p) if need[1] else None,
                    torch.zeros_like(p) if need[2] else None, None, None, None)
        # upstream g_t dt/df: grad_points is then g_t dt/dO, the sums g_t dt/dtheta
        u = (g_t * w).contiguous()
        out = ctx.renderer.sample_grad(ctx.frame, p, upstream=u, dist=False,
                                       grad_points=need[1] or need[2], grad_prims=need[0])
        g_o = out.grad_points
        return (_theta_grad(out.grad_prims, theta) if need[0] else None,
                g_o if need[1] else None, t[:, None] * g_o if need[2] else None,
                None, None, None)


def trace(renderer: Renderer, frame: Frame, theta, origins, dirs, min_cos: float = 1e-3):
    """Differentiable hit distance: returns (t (n,), hit (n,) bool) for the rays
    ``origins + t normalize(dirs)`` marched by sdf_trace through
    ``apply(frame.scene, theta)``.  With P = O + t D and G = grad f(P), the
    implicit-function theorem gives dt/dtheta = -(df/dtheta)(P) / (G . D), dt/dO =
    -G / (G . D) and dt/dD = t dt/dO; the directions are normalised here in torch,
    so the chain to `dirs` is torch's.  A ray carries no gradient, and `hit` is
    False, when it misses (t > max_dist), when t is NaN, or when it grazes the
    surface (|G . D| < min_cos |G|).  No kernel of its own: sdf_trace, then
    sdf_sample_grad for G, and one more sdf_sample_grad in the backward pass."""
    unit = dirs / dirs.norm(dim=1, keepdim=True)
    return _Trace.apply(theta, origins, unit, renderer, frame, float(min_cos))


__all__ = ["scene_tensor", "apply", "sample", "trace"]
