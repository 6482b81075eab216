"""Host-side renderer over the C-ABI (Python mirror of the C++ ``sdf::Renderer``).

One ``Renderer.render`` call is one frame of the reference's draw,
``gl->plot(sh, proj_mode)`` (/root/reference/Code/src/main.cpp:95): the scene,
camera, light and material go in, an RGBA float framebuffer comes out.  The
framebuffer lives in device memory allocated through PyTorch (plumbing only);
all arithmetic runs in the HIP kernels of ``libsdf3d.so``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

from . import abi
from .measure import Measure
from .scenes import Frame


def tiling(rank: int = 0, world: int = 1, block_rows: int = 8,
           frame_rows: bool = False, shares: tuple[int, int] = (1, 1)) -> abi.sdf_tiling:
    """Interleaved row-block tiling of `world` devices.

    shares = (a, b): per period of P = a + b (world - 1) blocks, rank 0 owns
    the first a blocks and rank r >= 1 the b blocks a + r - 1 + j (world - 1),
    j < b, interleaved with the other peers' (so a frame whose block count is
    not a multiple of P gives the last partial period to distinct ranks;
    (1, 1): device r owns blocks r, r + world, ...).  frame_rows: write the
    rows at their frame positions of a full-height buffer
    (SDF_TILING_FRAME_ROWS)."""
    a, b = shares
    if a < 1 or b < 1:
        raise ValueError(f"shares must be >= 1, got {shares}")
    t = abi.sdf_tiling()
    t.block_rows = block_rows
    t.block_stride = a + b * (world - 1)
    t.first_block = 0 if rank == 0 else a + rank - 1
    t.block_run = a if rank == 0 else b
    t.run_step = 1 if rank == 0 or b == 1 else world - 1
    t.flags = abi.TILING_FRAME_ROWS if frame_rows else 0
    return t


def buffer_rows(height: int, t: abi.sdf_tiling | None = None) -> int:
    """Rows of the output buffer of a render with tiling `t`."""
    if t is not None and t.flags & abi.TILING_FRAME_ROWS:
        return height
    return owned_rows(height, t)


def owned_rows(height: int, t: abi.sdf_tiling | None = None) -> int:
    n = abi.load_library().sdf_owned_rows(height, C.byref(t) if t is not None else None)
    if n < 0:
        abi.check(n, "sdf_owned_rows")
    return n


def torch_dtype(fmt: int):
    """torch element type of a framebuffer format."""
    import torch
    return {abi.FORMAT_RGBA32F: torch.float32, abi.FORMAT_RGBA16F: torch.float16,
            abi.FORMAT_RGBA8: torch.uint8, abi.FORMAT_RGB32F: torch.float32,
            abi.FORMAT_TILES: torch.uint8, abi.FORMAT_SHADE32F: torch.float32}[fmt]


def tiles_bytes(width: int, rows: int) -> int:
    """Capacity of a TILES stream (sdf_tiles_bytes)."""
    n = abi.load_library().sdf_tiles_bytes(width, rows)
    if n < 0:
        abi.check(int(n), "sdf_tiles_bytes")
    return int(n)


def tiles_stream_bytes(stream) -> int:
    """Meaningful prefix of a TILES stream on the host: table + used records."""
    import numpy as np
    used, n = np.frombuffer(bytes(stream[:8].cpu().numpy()), dtype=np.uint32)
    return (abi.TILES_HEADER_BYTES + 4 * int(n) + 15) // 16 * 16 + 16 * int(n) + int(used)


def channels(fmt: int) -> int:
    return abi.FORMAT_CHANNELS[fmt]


def samples(frame: Frame) -> int:
    """Sub-samples per axis of a frame's render (sdf_params.samples; 0 is 1)."""
    return max(int(frame.params.samples), 1)


def steps_shape(frame: Frame, t: abi.sdf_tiling | None = None) -> tuple[int, int, int]:
    """Shape of the steps tensor of ``Renderer.render(frame, t)``: one int2 per
    sample -- (S rows, S W, 2) with S x S supersampling, the layout of the
    S W x S H render's steps under the tiling with block_rows * S."""
    s = samples(frame)
    return (s * buffer_rows(frame.params.height, t), s * frame.params.width, 2)


class Hits(NamedTuple):
    """What ``Renderer.trace`` / ``trace_camera`` return (sdf_hits): device
    tensors, None for an output that was not asked for."""
    t: object
    steps: object
    normal: object
    prim: object


class Mesh(NamedTuple):
    """What ``Renderer.mesh`` returns: device tensors; `normal` and `prim` are
    None when not asked for; `counts` is the host copy of sdf_mesh_count's four
    numbers (vertices, triangles, bricks evaluated, bricks in all)."""
    verts: object
    tris: object
    normal: object
    prim: object
    counts: tuple


class Grad(NamedTuple):
    """What ``Renderer.sample_grad`` returns (sdf_grad_out): device tensors, None
    for an output that was not asked for; `grad_prims` is (16, 16), row i the
    sixteen slots of primitive i."""
    dist: object
    grad_points: object
    grad_prims: object


class Shade(NamedTuple):
    """What ``Renderer.shade_points`` returns (sdf_point_shade): device tensors,
    None for an output that was not asked for.  `rgba` (n, 4), `ao` (n,),
    `shadow` (n, L) and `steps` (n, L) int32 for the L lights, `material` (n, 9):
    the blended amb, dif and ref."""
    rgba: object
    ao: object
    shadow: object
    material: object
    steps: object


def grid(origin, cell, n, iso: float = 0.0, dense: bool = False) -> abi.sdf_grid:
    """The sdf_grid of n cells of size `cell` from `origin`; a scalar `cell` or
    `n` is used for all three axes."""
    cell = (cell,) * 3 if isinstance(cell, (int, float)) else tuple(cell)
    n = (n,) * 3 if isinstance(n, int) else tuple(n)
    g = abi.sdf_grid()
    for c in range(3):
        g.origin[c], g.cell[c], g.n[c] = float(origin[c]), float(cell[c]), int(n[c])
    g.iso = float(iso)
    g.flags = abi.MESH_DENSE if dense else 0
    return g


def mesh_sharp(sharp):
    """The sdf_mesh_sharp of ``Renderer.mesh``'s `sharp`: None or False none (a
    NULL pointer), True (4, 16), or ``(refine, iterations)``."""
    if sharp is None or sharp is False:
        return None
    refine, iterations = (4, 16) if sharp is True else sharp
    return abi.sdf_mesh_sharp(int(refine), int(iterations), 0, 0)


def _shading(frame: Frame, lights, materials, reflect=None):
    """The ctypes form of a call's `lights`, `materials` and `reflect` with
    ``Renderer.render``'s defaults -- the frame's light; the frame's material
    on every primitive (once for a Mandelbulb); a ``(bounces, strength)`` pair
    is the composite of that many bounces: (light array, its count, material
    array, its count, the sdf_reflect or None)."""
    if reflect is not None and not isinstance(reflect, abi.sdf_reflect):
        bounces, strength = reflect
        reflect = abi.sdf_reflect(int(bounces), float(strength), -1, 0)
    if materials is None:
        prims = frame.scene.kind == abi.SCENE_PRIMITIVES
        materials = [frame.material] * (frame.scene.count if prims else 1)
    materials = list(materials)
    marr = (abi.sdf_material * max(len(materials), 1))(*materials)
    lights = [frame.light] if lights is None else list(lights)
    larr = (abi.sdf_light * max(len(lights), 1))(*lights)
    return larr, len(lights), marr, len(materials), reflect


class Renderer:
    """Renders frames on one HIP device through ``sdf_render``."""

    def __init__(self, device=None):
        import torch
        self.torch = torch
        self.lib = abi.load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the renderer has no CPU path")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _on_device(self):
        """The HIP calls must run with this renderer's device current; enter
        a device context only when it is not (the context costs host time)."""
        import contextlib
        if self.torch.cuda.current_device() == self.device.index:
            return contextlib.nullcontext()
        return self.torch.cuda.device(self.device)

    def _stream(self, stream):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        return C.c_void_p(stream.cuda_stream)

    def alloc(self, frame: Frame, t: abi.sdf_tiling | None = None, steps: bool = False):
        rows = buffer_rows(frame.params.height, t)
        w = frame.params.width
        fmt = frame.params.output_format
        if fmt == abi.FORMAT_TILES:
            rgba = self.torch.empty((tiles_bytes(w, rows),), dtype=self.torch.uint8,
                                    device=self.device)
        else:
            rgba = self.torch.empty((rows, w, channels(fmt)), dtype=torch_dtype(fmt),
                                    device=self.device)
        st = (self.torch.empty(steps_shape(frame, t), dtype=self.torch.int32,
                               device=self.device) if steps else None)
        return rgba, st

    def schedule(self, rows: int, period: int = 1) -> "Schedule":
        """A render schedule for frames of `rows` packed rows (sdf_schedule):
        pass it to ``render(..., schedule=)`` to dispatch the rows' 8-row
        blocks costliest first (bit-identical output)."""
        return Schedule(self, rows, period)

    def render(self, frame: Frame, t: abi.sdf_tiling | None = None, out=None,
               steps=False, stream=None, schedule: "Schedule | None" = None,
               lights=None, light_flags: int = 0, materials=None, reflect=None, env=None):
        """Render the rows owned by tiling `t` (None = whole frame).

        Returns (rgba[rows, W, 4] float32, steps[rows, W, 2] int32 or None), both
        on the device, asynchronous on `stream` (default: torch's current).
        With ``frame.params.samples`` = S > 1 every pixel is the resolve of its
        S x S sub-samples and steps is (S rows, S W, 2): the sub-samples' counts.
        `schedule`: dispatch order of the row blocks (sdf_render_scheduled).
        `lights`: a sequence of 1 .. abi.MAX_LIGHTS ``abi.sdf_light`` lighting the
        frame together (sdf_render_lights; ``frame.light`` is then ignored), with
        `light_flags` (abi.LIGHTS_COLOR: every light scaled by its colour).
        `materials`: one ``abi.sdf_material`` per primitive of the scene (one for a
        Mandelbulb), blended along the CSG fold at every pixel
        (sdf_render_materials; ``frame.material`` is then ignored, and without
        `lights` the frame is lit by ``frame.light``); ``scenes.palette(n)`` gives
        n distinct ones.
        `reflect`: an ``abi.sdf_reflect`` or a ``(bounces, strength)`` pair: up to
        abi.MAX_BOUNCES mirror bounces per pixel, each surface's blended ``ref``
        times `strength` weighting what it reflects (sdf_render_reflect).  Without
        `materials` every primitive carries ``frame.material``.
        `env`: an ``abi.sdf_environment``: a sky for the rays that leave the scene
        and linear distance fog (sdf_render_env; ``scenes.sky()`` is a default
        one).  Without `reflect` it is rendered with no bounce."""
        torch = self.torch
        rows = buffer_rows(frame.params.height, t)
        w = frame.params.width
        if out is None:
            rgba, st = self.alloc(frame, t, steps is True)
        else:
            rgba = out
            st = None
        if isinstance(steps, torch.Tensor):
            st = steps
        if frame.params.output_format == abi.FORMAT_TILES:
            if rows and (rgba.dtype != torch.uint8 or rgba.numel() < tiles_bytes(w, rows)
                         or not rgba.is_contiguous() or rgba.device != self.device):
                raise ValueError(f"a TILES stream needs a contiguous uint8 tensor of "
                                 f">= {tiles_bytes(w, rows)} bytes on {self.device}")
        else:
            dt = torch_dtype(frame.params.output_format)
            ch = channels(frame.params.output_format)
            if tuple(rgba.shape) != (rows, w, ch) or rgba.dtype != dt \
                    or not rgba.is_contiguous() or rgba.device != self.device:
                raise ValueError(f"rgba must be a contiguous {dt} ({rows}, {w}, {ch}) tensor "
                                 f"on {self.device}")
        sshape = steps_shape(frame, t)
        if st is not None and (tuple(st.shape) != sshape or st.dtype != torch.int32
                               or not st.is_contiguous()):
            raise ValueError(f"steps must be a contiguous int32 {sshape} tensor")
        with self._on_device():
            head = (C.byref(frame.scene), C.byref(frame.camera))
            tail = (C.byref(frame.params), C.byref(t) if t is not None else None,
                    C.c_void_p(rgba.data_ptr()),
                    C.c_void_p(st.data_ptr()) if st is not None else None)
            sched = schedule.handle if schedule is not None else None
            if env is not None and reflect is None:
                reflect = abi.sdf_reflect(0, 1.0, -1, 0)
            name = "sdf_render"
            if reflect is not None or materials is not None or lights is not None:
                larr, nl, marr, nm, reflect = _shading(frame, lights, materials, reflect)
                lit = (*head, larr, nl, int(light_flags))
                if env is not None:
                    name, args = "sdf_render_env", (*lit, marr, nm, C.byref(reflect), C.byref(env))
                elif reflect is not None:
                    name, args = "sdf_render_reflect", (*lit, marr, nm, C.byref(reflect))
                elif materials is not None:
                    name, args = "sdf_render_materials", (*lit, marr, nm)
                else:
                    name, args = "sdf_render_lights", (*lit, C.byref(frame.material))
                rc = getattr(self.lib, name)(*args, *tail, sched, self._stream(stream))
            else:
                args = (*head, C.byref(frame.light), C.byref(frame.material), *tail)
                if schedule is None:
                    rc = self.lib.sdf_render(*args, self._stream(stream))
                else:
                    rc = self.lib.sdf_render_scheduled(*args, sched, self._stream(stream))
        abi.check(rc, name)
        return rgba, st

    def render_multi(self, frame: Frame, devices, shares=(0, 0), out=None, stream=None):
        """One RGBA32F frame rendered across `devices` (device indices of this
        process, this renderer's device first) through sdf_render_multi: the
        root renders its rows in place and decodes the other devices' TILES
        streams through peer-mapped memory.  Returns the (H, W, 4) frame on
        this renderer's device, asynchronous on `stream`."""
        torch = self.torch
        devs = [int(d) for d in devices]
        if not devs or devs[0] != self.device.index:
            raise ValueError("devices[0] must be this renderer's device")
        p = frame.params
        if out is None:
            out = torch.empty((p.height, p.width, 4), dtype=torch.float32, device=self.device)
        if (tuple(out.shape) != (p.height, p.width, 4) or out.dtype != torch.float32
                or not out.is_contiguous() or out.device != self.device):
            raise ValueError("out must be a contiguous float32 (H, W, 4) tensor on the root")
        arr = (C.c_int32 * len(devs))(*devs)
        with self._on_device():
            rc = self.lib.sdf_render_multi(
                C.byref(frame.scene), C.byref(frame.camera), C.byref(frame.light),
                C.byref(frame.material), C.byref(frame.params), len(devs), arr,
                int(shares[0]), int(shares[1]), C.c_void_p(out.data_ptr()), self._stream(stream))
        abi.check(rc, "sdf_render_multi")
        return out

    def render_frames(self, frame: Frame, cameras, outs, steps=None, stream=None):
        """Whole frames of `frame`'s scene, frame i through cameras[i] into
        outs[i] (and its iteration counts into steps[i]), by the persistent
        frame-sequence kernel (sdf_render_frames): the same pixels as one
        ``render`` per camera.  Asynchronous on `stream`; returns `outs`."""
        torch = self.torch
        n = len(cameras)
        if len(outs) != n or (steps is not None and len(steps) != n):
            raise ValueError("one output (and one steps buffer) per camera")
        p = frame.params
        if p.output_format == abi.FORMAT_TILES:
            raise ValueError("frame sequences take plain formats, not TILES")
        dt, ch = torch_dtype(p.output_format), channels(p.output_format)
        for o in outs:
            if tuple(o.shape) != (p.height, p.width, ch) or o.dtype != dt \
                    or not o.is_contiguous() or o.device != self.device:
                raise ValueError(f"outputs must be contiguous {dt} ({p.height}, {p.width}, {ch}) "
                                 f"tensors on {self.device}")
        for s in steps or ():
            if tuple(s.shape) != (p.height, p.width, 2) or s.dtype != torch.int32 \
                    or not s.is_contiguous() or s.device != self.device:
                raise ValueError("steps must be contiguous int32 (H, W, 2) tensors")
        cams = (abi.sdf_camera * max(n, 1))(*cameras)
        ptrs = (C.c_void_p * max(n, 1))(*[o.data_ptr() for o in outs])
        sptrs = (C.c_void_p * max(n, 1))(*[s.data_ptr() for s in steps]) if steps else None
        with self._on_device():
            rc = self.lib.sdf_render_frames(
                C.byref(frame.scene), cams, n, C.byref(frame.light), C.byref(frame.material),
                C.byref(frame.params), ptrs, sptrs, self._stream(stream))
        abi.check(rc, "sdf_render_frames")
        return outs

    # ---- queries (sdf_abi.h "Queries") --------------------------------------
    def _n3(self, x, what: str):
        torch = self.torch
        if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2
                or x.shape[1] != 3 or not x.is_contiguous() or x.device != self.device):
            raise ValueError(f"{what} must be a contiguous float32 (n, 3) tensor on {self.device}")
        return x

    def _hits(self, shape, t: bool, steps: bool, normal: bool, prim: bool):
        torch = self.torch
        if not (t or steps or normal or prim):
            raise ValueError("a query needs at least one output")

        def new(want, tail, dtype):
            return torch.empty((*shape, *tail), dtype=dtype, device=self.device) if want else None
        out = Hits(new(t, (), torch.float32), new(steps, (), torch.int32),
                   new(normal, (3,), torch.float32), new(prim, (), torch.int32))
        ptr = [C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None for x in out]
        return out, abi.sdf_hits(*ptr)

    def trace(self, frame: Frame, origins, dirs, normal: bool = True, prim: bool = True,
              stream=None, t: bool = True, steps: bool = True) -> "Hits":
        """March n rays through ``frame.scene`` (sdf_trace): ray i starts at
        ``origins[i]`` and runs along ``dirs[i]`` (any non-zero length; the
        kernel normalises) with the frame's max_steps, max_dist, eps, normal
        mode, precision and dispatch.  `origins` and `dirs` are contiguous
        float32 (n, 3) tensors on this renderer's device, used in place.
        Returns ``Hits(t, steps, normal, prim)``: the march's distance (n,), its
        iteration count (n,) int32, the normal at the hit (n, 3) -- zeros on a
        miss (t > max_dist) -- and the index of the primitive that owns the
        hit (n,) int32, -1 on a miss; an output that was not asked for is
        None.  Asynchronous on `stream`."""
        o, d = self._n3(origins, "origins"), self._n3(dirs, "dirs")
        if o.shape != d.shape:
            raise ValueError("origins and dirs must have the same shape")
        n = o.shape[0]
        out, hits = self._hits((n,), t, steps, normal, prim)
        if n == 0:
            return out
        with self._on_device():
            rc = self.lib.sdf_trace(C.byref(frame.scene), C.byref(frame.params),
                                    C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), n,
                                    C.byref(hits), self._stream(stream))
        abi.check(rc, "sdf_trace")
        return out

    def trace_camera(self, frame: Frame, normal: bool = True, prim: bool = True, stream=None,
                     t: bool = True, steps: bool = True) -> "Hits":
        """``trace`` for the rays ``render`` marches (sdf_trace_camera): entry
        [y, x] is pixel (x, y)'s ray, so `t` is a depth map, `normal` a normal
        map and `prim` a segmentation map of the frame, and `steps` equals
        ``render(..., steps=True)[1][..., 0]``.  Tensors are shaped (H, W) and
        (H, W, 3).  One ray per pixel: ``frame.params.samples`` > 1 is refused."""
        p = frame.params
        out, hits = self._hits((p.height, p.width), t, steps, normal, prim)
        with self._on_device():
            rc = self.lib.sdf_trace_camera(C.byref(frame.scene), C.byref(frame.camera),
                                           C.byref(p), C.byref(hits), self._stream(stream))
        abi.check(rc, "sdf_trace_camera")
        return out

    def sample(self, frame: Frame, points, normal: bool = False, stream=None):
        """The scene's signed distance at n points (sdf_sample): `points` is a
        contiguous float32 (n, 3) tensor on this renderer's device.  Returns
        (dist (n,), normal (n, 3) or None), the normal with the frame's normal
        mode and normal_eps.  Asynchronous on `stream`."""
        torch = self.torch
        pts = self._n3(points, "points")
        n = pts.shape[0]
        dist = torch.empty((n,), dtype=torch.float32, device=self.device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=self.device) if normal else None
        if n == 0:
            return dist, nrm
        with self._on_device():
            rc = self.lib.sdf_sample(C.byref(frame.scene), C.byref(frame.params),
                                     C.c_void_p(pts.data_ptr()), n, C.c_void_p(dist.data_ptr()),
                                     C.c_void_p(nrm.data_ptr()) if normal else None,
                                     self._stream(stream))
        abi.check(rc, "sdf_sample")
        return dist, nrm

    # ---- gradients (sdf_abi.h "Gradients") ----------------------------------
    def sample_grad(self, frame: Frame, points, upstream=None, dist: bool = False,
                    grad_points: bool = True, grad_prims: bool = True, stream=None) -> "Grad":
        """The scene function's analytic gradients at n points (sdf_sample_grad):
        `points` is a contiguous float32 (n, 3) tensor on this renderer's device,
        `upstream` a contiguous float32 (n,) tensor of weights g there (None:
        every g_i = 1).  Returns ``Grad(dist (n,), grad_points (n, 3) = g_i
        df/dp, grad_prims (16, 16))``: row i of `grad_prims` holds, in the slots of
        ``sdf_primitive`` (2: k, 4 + j: p[j]), the sums over the points of g_i
        df/d(parameter), zeros elsewhere.  An output that was not asked for is
        None.  With n = 0 nothing is launched and `grad_prims` is all zero.
        Asynchronous on `stream`."""
        torch = self.torch
        pts = self._n3(points, "points")
        n = pts.shape[0]
        if upstream is not None and (
                not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.float32
                or tuple(upstream.shape) != (n,) or not upstream.is_contiguous()
                or upstream.device != self.device):
            raise ValueError(f"upstream must be a contiguous float32 ({n},) tensor on {self.device}")
        if not (dist or grad_points or grad_prims):
            raise ValueError("sample_grad needs at least one output")

        def new(want, shape):
            return torch.empty(shape, dtype=torch.float32, device=self.device) if want else None
        out = Grad(new(dist, (n,)), new(grad_points, (n, 3)),
                   new(grad_prims, (abi.SDF_MAX_PRIMS, 16)))
        if n == 0:
            if out.grad_prims is not None:
                out.grad_prims.zero_()
            return out
        nbytes = int(self.lib.sdf_grad_workspace_bytes(n)) if grad_prims else 0
        if nbytes < 0:
            abi.check(nbytes, "sdf_grad_workspace_bytes")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device) if grad_prims else None
        go = abi.sdf_grad_out(*[C.c_void_p(x.data_ptr()) if x is not None else None for x in out])
        with self._on_device():
            rc = self.lib.sdf_sample_grad(
                C.byref(frame.scene), C.byref(frame.params), C.c_void_p(pts.data_ptr()), n,
                C.c_void_p(upstream.data_ptr()) if upstream is not None else None, C.byref(go),
                C.c_void_p(ws.data_ptr()) if ws is not None else None, nbytes,
                self._stream(stream))
        abi.check(rc, "sdf_sample_grad")
        if ws is not None and stream is not None:
            ws.record_stream(stream)   # the workspace is in use on `stream` past this call
        return out

    # ---- isosurface meshes (sdf_abi.h "Meshes") -----------------------------
    def mesh(self, frame: Frame, origin, cell, n, iso: float = 0.0, normal: bool = False,
             prim: bool = False, dense: bool = False, stream=None, sharp=None) -> "Mesh":
        """The level set ``f(p) = iso`` of ``frame.scene`` inside the grid of
        `n` cells of size `cell` from `origin`, as an indexed triangle mesh
        (sdf_mesh_count, then sdf_mesh_emit into buffers sized from its counts;
        the host waits for the counts in between).  Returns ``Mesh(verts (nv, 3)
        float32, tris (nt, 3) int32, normal (nv, 3) or None, prim (nv,) int32 or
        None, counts)``.  `dense` evaluates every brick (SDF_MESH_DENSE); the
        mesh is the same either way.  `sharp` places the vertices on the
        scene's edges and corners instead of chamfering them
        (sdf_mesh_emit_sharp, "Sharp meshes"): True for 4 refinement steps per
        crossing and 16 steps of the fit, or ``(refine, iterations)``; the
        triangles are the same.  Not for a Mandelbulb."""
        torch = self.torch
        g = grid(origin, cell, n, iso, dense)
        sp = mesh_sharp(sharp)
        nbytes = int(self.lib.sdf_mesh_workspace_bytes(C.byref(g)))
        if nbytes < 0:
            abi.check(nbytes, "sdf_mesh_workspace_bytes")
        abi.check(self.lib.sdf_validate_mesh_sharp(C.byref(frame.scene), C.byref(frame.params),
                                                   C.byref(g), sp), "sdf_validate_mesh_sharp")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        counts = torch.empty((4,), dtype=torch.int64, device=self.device)
        with self._on_device():
            rc = self.lib.sdf_mesh_count(C.byref(frame.scene), C.byref(frame.params), C.byref(g),
                                         C.c_void_p(ws.data_ptr()), nbytes,
                                         C.c_void_p(counts.data_ptr()), self._stream(stream))
            abi.check(rc, "sdf_mesh_count")
            # the copy is ordered behind the count only on the stream it ran on
            if stream is not None:
                torch.cuda.synchronize(self.device)
            nv, nt, evaluated, bricks = (int(x) for x in counts.cpu().tolist())
            verts = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
            tris = torch.empty((nt, 3), dtype=torch.int32, device=self.device)
            nrm = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if normal else None
            own = torch.empty((nv,), dtype=torch.int32, device=self.device) if prim else None

            def ptr(x):
                return C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None
            out = abi.sdf_mesh_out(ptr(verts), nv, ptr(tris), nt, ptr(nrm), ptr(own))
            rc = self.lib.sdf_mesh_emit_sharp(C.byref(frame.scene), C.byref(frame.params),
                                              C.byref(g), sp, C.c_void_p(ws.data_ptr()), nbytes,
                                              C.byref(out), self._stream(stream))
            abi.check(rc, "sdf_mesh_emit_sharp")
            if stream is not None:
                stream.synchronize()   # the workspace is released on return
        return Mesh(verts, tris, nrm, own, (nv, nt, evaluated, bricks))

    # ---- measures (sdf_abi.h "Measures") --------------------------------------
    def measure(self, frame: Frame, origin, cell, n, iso: float = 0.0, owners: bool = False,
                dense: bool = False, stream=None) -> Measure:
        """Volume, centroid, inertia and bounds of the solid ``f(p) < iso`` of
        ``frame.scene`` inside the grid of `n` cells of size `cell` from `origin`,
        one sample per cell centre (sdf_measure).  Returns a
        ``sdf3d_amd.measure.Measure`` of the call's integer rows and counts: row
        0 the whole solid, with `owners` a row per owning primitive besides (for
        ``select`` and per-primitive densities).  `dense` evaluates every brick
        (SDF_MESH_DENSE); the rows are the same either way.  The host waits for
        the rows."""
        torch = self.torch
        g = grid(origin, cell, n, iso, dense)
        flags = abi.MEASURE_OWNERS if owners else 0
        abi.check(self.lib.sdf_validate_measure(C.byref(frame.scene), C.byref(frame.params),
                                                C.byref(g), flags), "sdf_validate_measure")
        nbytes = int(self.lib.sdf_measure_workspace_bytes(C.byref(g), flags))
        if nbytes < 0:
            abi.check(nbytes, "sdf_measure_workspace_bytes")
        rows = abi.MEASURE_ROWS if owners else 1
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        moments = torch.empty((rows, abi.MEASURE_SLOTS), dtype=torch.int64, device=self.device)
        counts = torch.empty((4,), dtype=torch.int64, device=self.device)
        with self._on_device():
            rc = self.lib.sdf_measure(C.byref(frame.scene), C.byref(frame.params), C.byref(g), flags,
                                      C.c_void_p(ws.data_ptr()), nbytes,
                                      C.c_void_p(moments.data_ptr()),
                                      C.c_void_p(counts.data_ptr()), self._stream(stream))
            abi.check(rc, "sdf_measure")
            if stream is not None:
                stream.synchronize()   # the copies below run on the current stream
            return Measure(moments.cpu().numpy(), counts.cpu().tolist(), tuple(g.origin),
                           tuple(g.cell), tuple(g.n))

    # ---- caller-supplied rays (sdf_abi.h "Rays") ----------------------------
    def render_rays(self, frame: Frame, origins, dirs, unit: bool = False, out=None,
                    steps=False, lights=None, light_flags: int = 0, materials=None,
                    reflect=None, env=None, stream=None):
        """Shade n rays of the caller's own through ``frame.scene``
        (sdf_render_rays): ray i starts at ``origins[i]`` and runs along
        ``dirs[i]`` -- any non-zero length, the kernel normalises; with `unit`
        (SDF_RAYS_UNIT) the directions are unit vectors used as given, as
        ``camera_rays`` returns them.  `origins` and `dirs` are contiguous
        float32 (n, 3) tensors on this renderer's device, used in place.
        `lights`, `light_flags`, `materials`, `reflect` and `env` are
        ``render``'s, with its defaults; the frame's camera, size and samples
        play no part.  Returns (rgba (n, ch) of ``frame.params.output_format``,
        steps (n, 2) int32 or None).  A ray whose direction has no finite
        normalisation is inactive: all-zero output, alpha included.  A wave
        shades 64 consecutive rays, so order them in coherent groups of 64.
        Asynchronous on `stream`."""
        torch = self.torch
        o, d = self._n3(origins, "origins"), self._n3(dirs, "dirs")
        if o.shape != d.shape:
            raise ValueError("origins and dirs must have the same shape")
        n = o.shape[0]
        fmt = frame.params.output_format
        if fmt not in (abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8,
                       abi.FORMAT_RGB32F):
            raise ValueError("render_rays writes RGBA32F, RGBA16F, RGBA8 or RGB32F pixels")
        dt, ch = torch_dtype(fmt), channels(fmt)
        rgba = torch.empty((n, ch), dtype=dt, device=self.device) if out is None else out
        if tuple(rgba.shape) != (n, ch) or rgba.dtype != dt or not rgba.is_contiguous() \
                or rgba.device != self.device:
            raise ValueError(f"out must be a contiguous {dt} ({n}, {ch}) tensor on {self.device}")
        st = steps if isinstance(steps, torch.Tensor) else (
            torch.empty((n, 2), dtype=torch.int32, device=self.device) if steps else None)
        if st is not None and (tuple(st.shape) != (n, 2) or st.dtype != torch.int32
                               or not st.is_contiguous() or st.device != self.device):
            raise ValueError(f"steps must be a contiguous int32 ({n}, 2) tensor on {self.device}")
        arr, nl, marr, nm, reflect = _shading(frame, lights, materials, reflect)
        rays = abi.sdf_rays(o.data_ptr() if n else None, d.data_ptr() if n else None, n,
                            abi.RAYS_UNIT if unit else 0, 0)
        with self._on_device():
            rc = self.lib.sdf_render_rays(
                C.byref(frame.scene), arr, nl, int(light_flags), marr, nm,
                C.byref(reflect) if reflect is not None else None,
                C.byref(env) if env is not None else None, C.byref(frame.params),
                C.byref(rays), C.c_void_p(rgba.data_ptr()) if n else None,
                C.c_void_p(st.data_ptr()) if st is not None and n else None,
                self._stream(stream))
        abi.check(rc, "sdf_render_rays")
        return rgba, st

    # ---- shading at caller-supplied points (sdf_abi.h "Points") -------------
    def shade_points(self, frame: Frame, points, normals=None, eye=None, lift: float = 0.0,
                     lights=None, materials=None, rgba: bool = True, ao: bool = False,
                     shadow: bool = False, material: bool = False, steps: bool = False,
                     stream=None, light_flags: int = 0) -> "Shade":
        """Lights, shadows, occlusion and materials of ``frame.scene`` at n points
        of the caller's own (sdf_shade_points), without a primary march: `points`
        is a contiguous float32 (n, 3) tensor on this renderer's device, `normals`
        the same (used as given) or None (the normal is evaluated at the point).
        `eye` (three floats) switches the specular term on; without it there is
        none.  `lift` moves each point along its normal before anything is
        shaded (vertices of ``mesh`` lie up to half a cell diagonal inside the
        surface).  `lights`, `light_flags` and `materials` are ``render``'s, with
        its defaults.  Returns ``Shade(rgba, ao, shadow, material, steps)``, None
        for what was not asked for; what is not asked for is not computed.  A
        wave shades 64 consecutive points.  Asynchronous on `stream`."""
        torch = self.torch
        pts = self._n3(points, "points")
        n = pts.shape[0]
        nrm = None if normals is None else self._n3(normals, "normals")
        if nrm is not None and nrm.shape != pts.shape:
            raise ValueError("points and normals must have the same shape")
        if not (rgba or ao or shadow or material or steps):
            raise ValueError("shade_points needs at least one output")
        arr, nl, marr, nm, _ = _shading(frame, lights, materials)

        def new(want, tail, dtype=torch.float32):
            return torch.empty((n, *tail), dtype=dtype, device=self.device) if want else None
        out = Shade(new(rgba, (4,)), new(ao, ()), new(shadow, (nl,)), new(material, (9,)),
                    new(steps, (nl,), torch.int32))
        if n == 0:
            return out
        p = abi.sdf_points()
        p.points = pts.data_ptr()
        p.normals = nrm.data_ptr() if nrm is not None else None
        p.n = n
        if eye is not None:
            p.flags = abi.POINTS_EYE
            for c in range(3):
                p.eye[c] = float(eye[c])
        p.lift = float(lift)
        ps = abi.sdf_point_shade(*[C.c_void_p(x.data_ptr()) if x is not None else None
                                   for x in out])
        with self._on_device():
            rc = self.lib.sdf_shade_points(C.byref(frame.scene), arr, nl, int(light_flags), marr,
                                           nm, C.byref(frame.params), C.byref(p),
                                           C.byref(ps), self._stream(stream))
        abi.check(rc, "sdf_shade_points")
        return out

    def bake(self, frame: Frame, mesh: "Mesh", cell, eye=None, lift=None, lights=None,
             materials=None, stream=None, light_flags: int = 0):
        """Vertex colours of a ``Mesh`` of ``frame.scene`` extracted with cells of
        size `cell` (a scalar, or one per axis): ``shade_points`` at the vertices,
        with the mesh's normals when it has them.  The default `lift` is the
        length of the cell diagonal: a surface-nets vertex lies within half a
        diagonal of the surface, so one diagonal puts it outside for a field
        whose Lipschitz constant is 1.  A mesh extracted with `sharp` has its
        vertices on the surface and needs less, but a ``Mesh`` does not say how
        it was made, so the default is the same: pass a smaller `lift` for one.
        Returns a float32 (V, 4) tensor."""
        cell = (cell,) * 3 if isinstance(cell, (int, float)) else tuple(cell)
        if lift is None:
            lift = math.sqrt(sum(float(c) * float(c) for c in cell))
        return self.shade_points(frame, mesh.verts, normals=mesh.normal, eye=eye, lift=lift,
                                 lights=lights, materials=materials, stream=stream,
                                 light_flags=light_flags).rgba

    def camera_rays(self, frame: Frame, stream=None):
        """The rays ``render`` marches (sdf_camera_rays): (origins, dirs), each a
        float32 (H, W, 3) tensor whose entry [y, x] is pixel (x, y)'s eye and
        unit direction in the frame's precision -- a starting point to perturb,
        and with ``render_rays(..., unit=True)`` on their (H W, 3) views the
        frame ``render`` gives.  One ray per pixel: ``frame.params.samples`` > 1
        is refused.  Asynchronous on `stream`."""
        torch = self.torch
        p = frame.params
        o = torch.empty((p.height, p.width, 3), dtype=torch.float32, device=self.device)
        d = torch.empty((p.height, p.width, 3), dtype=torch.float32, device=self.device)
        with self._on_device():
            rc = self.lib.sdf_camera_rays(C.byref(frame.camera), C.byref(p),
                                          C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                          self._stream(stream))
        abi.check(rc, "sdf_camera_rays")
        return o, d

    def heatmap(self, steps, which: int = 0, max_steps: int = 128, fmt: int = abi.FORMAT_RGBA8,
                out=None, stream=None):
        """Turbo-coloured view of a `steps` tensor (rows, W, 2) from render()."""
        torch = self.torch
        if steps.dtype != torch.int32 or steps.shape[-1] != 2 or not steps.is_contiguous():
            raise ValueError("steps must be a contiguous int32 (..., 2) tensor")
        count = steps.numel() // 2
        if out is None:
            out = torch.empty((*steps.shape[:-1], channels(fmt)), dtype=torch_dtype(fmt),
                              device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdf_heatmap(C.c_void_p(steps.data_ptr()), count, which, max_steps,
                                      fmt, C.c_void_p(out.data_ptr()), self._stream(stream))
        abi.check(rc, "sdf_heatmap")
        return out

    def deinterleave(self, parts, nparts: int, part_stride_rows: int, width: int,
                     height: int, block_rows: int = 8, out=None, stream=None,
                     fmt: int | None = None):
        """Scatter gathered packed row blocks (nparts x part_stride_rows rows)
        into a full (height, width, 4) frame on this device."""
        torch = self.torch
        if fmt is None:
            fmt = {torch.float32: abi.FORMAT_RGBA32F, torch.float16: abi.FORMAT_RGBA16F,
                   torch.uint8: abi.FORMAT_RGBA8}[parts.dtype]
            if parts.shape[-1] == 3:
                fmt = abi.FORMAT_RGB32F
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch_dtype(fmt), device=self.device)
        if parts.numel() < nparts * part_stride_rows * width * channels(fmt) \
                or not parts.is_contiguous() or parts.dtype != torch_dtype(fmt) \
                or out.dtype != parts.dtype or tuple(out.shape) != (height, width, 4) \
                or not out.is_contiguous():
            raise ValueError("parts/frame buffers of the wrong size, layout or format")
        with torch.cuda.device(self.device):
            rc = self.lib.sdf_deinterleave(C.c_void_p(parts.data_ptr()), nparts,
                                           part_stride_rows, width, height, block_rows, fmt,
                                           C.c_void_p(out.data_ptr()), self._stream(stream))
        abi.check(rc, "sdf_deinterleave")
        return out

    def tiles_decode(self, parts, nparts: int, part_stride: int, width: int, height: int,
                     block_rows: int = 8, out=None, stream=None, tilings=None):
        """Decode `nparts` TILES streams (uint8, pitch `part_stride` bytes; part
        r from tiling {block_rows, r, nparts}, or from tilings[r] when given)
        into a (height, width, 4) float32 frame on this device
        (sdf_tiles_decode / sdf_tiles_decode_tilings)."""
        torch = self.torch
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.device)
        if parts.dtype != torch.uint8 or not parts.is_contiguous() \
                or parts.numel() < nparts * part_stride or out.dtype != torch.float32 \
                or tuple(out.shape) != (height, width, 4) or not out.is_contiguous():
            raise ValueError("TILES parts / RGBA32F frame of the wrong size, layout or type")
        with self._on_device():
            if tilings is None:
                rc = self.lib.sdf_tiles_decode(C.c_void_p(parts.data_ptr()), nparts, part_stride,
                                               width, height, block_rows,
                                               C.c_void_p(out.data_ptr()), self._stream(stream))
            else:
                if len(tilings) != nparts:
                    raise ValueError("one tiling per part")
                arr = (abi.sdf_tiling * nparts)(*tilings)
                rc = self.lib.sdf_tiles_decode_tilings(C.c_void_p(parts.data_ptr()), nparts,
                                                       part_stride, arr, width, height,
                                                       C.c_void_p(out.data_ptr()),
                                                       self._stream(stream))
        abi.check(rc, "sdf_tiles_decode")
        return out

    def tiles_decode_checked(self, parts, nparts: int, part_stride: int, width: int, height: int,
                             tilings, used=None, out=None, status=None, stream=None):
        """sdf_tiles_decode_checked: the decode of tiles_decode(tilings=...)
        for streams that crossed a wire.  `used`: each part's expected data
        bytes (-1: its header's); `status`: a uint32 device tensor of nparts
        words (zeroed here) that receives each part's SDF_TILES_BAD_* bits,
        or None for a synchronous call that raises (SDF_E_COMM) when some
        part was malformed.  Returns (frame, status)."""
        torch = self.torch
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.device)
        if parts.dtype != torch.uint8 or not parts.is_contiguous() \
                or parts.numel() < nparts * part_stride or out.dtype != torch.float32 \
                or tuple(out.shape) != (height, width, 4) or not out.is_contiguous() \
                or len(tilings) != nparts:
            raise ValueError("TILES parts / RGBA32F frame of the wrong size, layout or type")
        if status is not None:
            if status.dtype != torch.int32 or status.numel() < nparts or not status.is_contiguous():
                raise ValueError("status: nparts int32 words (holding uint32 codes)")
            status.zero_()
        arr = (abi.sdf_tiling * nparts)(*tilings)
        u = None if used is None else (C.c_int64 * nparts)(*[int(x) for x in used])
        with self._on_device():
            rc = self.lib.sdf_tiles_decode_checked(
                C.c_void_p(parts.data_ptr()), nparts, part_stride, arr, u, width, height,
                C.c_void_p(out.data_ptr()),
                None if status is None else C.c_void_p(status.data_ptr()), self._stream(stream))
        abi.check(rc, "sdf_tiles_decode_checked")
        return out, status


class Schedule:
    """sdf_schedule: the dispatch order of a frame's 8-row blocks, costliest
    first, learnt from the cycles the kernels measured in earlier frames
    (include/sdf_abi.h).  One per stream; ``close()`` frees it."""

    def __init__(self, renderer: "Renderer", rows: int, period: int = 1):
        self.lib = renderer.lib
        self.handle = C.c_void_p()
        with renderer._on_device():
            abi.check(self.lib.sdf_schedule_create(int(rows), int(period), C.byref(self.handle)),
                      "sdf_schedule_create")

    def order(self) -> list[int]:
        """blockIdx.y -> 8-row block ([] until the first cost snapshot landed)."""
        buf = (C.c_int32 * 512)()
        n = self.lib.sdf_schedule_order(self.handle, buf, 512)
        if n < 0:
            abi.check(n, "sdf_schedule_order")
        return list(buf[:n])

    def close(self) -> None:
        if self.handle:
            self.lib.sdf_schedule_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass
