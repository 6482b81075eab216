"""Reference of shading at caller-supplied points (include/sdf_abi.h "Points",
sdf_shade_points) and what its tests share.

The reference itself is C over the CPU oracle (tests/points_ref.c, compiled on
first use like materials_ref; sdf3d_amd/build.py build_points_ref builds it with
the rest).  `shade` runs it on host arrays; `hit_points` forms the points a
render's primary march ends on, P_0 = O_0 + D_0 d, in unfused fp32 from a
distance map and the camera's rays, the way the render forms them.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import NamedTuple

import numpy as np

import oracle
from sdf3d_amd import abi

f32 = np.float32
HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "build" / "libpoints_ref.so"
_lib = None


class RefShade(NamedTuple):
    rgba: np.ndarray       # (n, 4)
    ao: np.ndarray         # (n,)
    shadow: np.ndarray     # (n, L)
    material: np.ndarray   # (n, 9)
    steps: np.ndarray      # (n, L) int32
    dif: np.ndarray        # (n, L): clamp(N . incident, 0, 1) sh_i


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        from sdf3d_amd import build
        build.build_points_ref(verbose=False)
    lib = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    lib.sdf_points_ref_shade.argtypes = [
        P(abi.sdf_scene), P(abi.sdf_light), C.c_int, C.c_int, P(abi.sdf_material), C.c_int,
        P(abi.sdf_params), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_float,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_int]
    lib.sdf_points_ref_shade.restype = C.c_int
    _lib = lib
    return lib


def default_materials(frame):
    prims = frame.scene.kind == abi.SCENE_PRIMITIVES
    return [frame.material] * (frame.scene.count if prims else 1)


def shade(frame, points, normals=None, eye=None, lift=0.0, lights=None, light_flags=0,
          materials=None, steps=None) -> RefShade:
    """The reference's outputs for `points` (n, 3) with ``Renderer.shade_points``'s
    arguments.  `steps` ((n, L) int32): light i's shadow march is replayed at
    that count instead of running to its own break."""
    pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n = pts.shape[0]
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=f32).reshape(n, 3)
    lights = [frame.light] if lights is None else list(lights)
    materials = default_materials(frame) if materials is None else list(materials)
    nl = len(lights)
    larr = (abi.sdf_light * nl)(*lights)
    marr = (abi.sdf_material * len(materials))(*materials)
    e = None if eye is None else np.asarray(eye, dtype=f32).reshape(3).copy()
    force = None if steps is None else np.ascontiguousarray(steps, dtype=np.int32).reshape(n, nl)
    out = RefShade(np.empty((n, 4), f32), np.empty((n,), f32), np.empty((n, nl), f32),
                   np.empty((n, 9), f32), np.empty((n, nl), np.int32), np.empty((n, nl), f32))

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = load().sdf_points_ref_shade(
        C.byref(frame.scene), larr, nl, int(light_flags), marr, len(materials),
        C.byref(frame.params), ptr(pts), ptr(nrm), n, ptr(e), float(f32(lift)), ptr(force),
        ptr(out.rgba), ptr(out.ao), ptr(out.shadow), ptr(out.material), ptr(out.steps),
        ptr(out.dif), oracle.default_threads())
    if rc != 0:
        raise RuntimeError(f"points reference failed: {rc}")
    return out


def camera_rays(frame):
    """(O_0 (3,), D_0 [H, W, 3]) of the frame's pixels as the oracle's render
    loop forms them (oracle_core.h render_rows), in unfused fp32."""
    p = frame.params
    u = oracle.uniforms(frame.camera, p)
    W, H = p.width, p.height
    with np.errstate(all="ignore"):
        qx = ((2 * np.arange(W) + 1).astype(f32) / f32(W) - f32(1.0)).astype(f32)
        qy = ((2 * np.arange(H) + 1).astype(f32) / f32(H) - f32(1.0)).astype(f32)
        x = np.broadcast_to((qx * f32(u["aspect"])).astype(f32)[None, :], (H, W))
        y = np.broadcast_to(qy[:, None], (H, W))
        z = np.full((H, W), f32(u["focal"]), dtype=f32)
        r0 = _normalize(x, y, z)
        m = u["inv_view"].astype(f32)
        r1 = [((m[0 + c] * r0[0] + m[4 + c] * r0[1]).astype(f32) + m[8 + c] * r0[2]).astype(f32)
              + (m[12 + c] * f32(0.0)) for c in range(3)]
        ray = _normalize(*[a.astype(f32) for a in r1])
    return u["cam"].astype(f32), np.stack(ray, axis=-1).astype(f32)


def _normalize(x, y, z):
    l = np.sqrt(((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32),
                dtype=f32)
    return (x / l).astype(f32), (y / l).astype(f32), (z / l).astype(f32)


def hit_points(cam, rays, d):
    """P_0 = O_0 + D_0 d per pixel in unfused fp32: RN(cam.c + RN(ray.c d))."""
    d = np.asarray(d, dtype=f32)[..., None]
    with np.errstate(all="ignore"):
        return (np.asarray(cam, f32) + (np.asarray(rays, f32) * d).astype(f32)).astype(f32)
