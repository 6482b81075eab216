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

import materials_ref as MR
import oracle
from cases import LIGHTS, points_scene
from gpu_support import fenced, same, untouched
from sdf3d_amd import abi, scenes

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


# ---- the kernel's side: what tests/test_gpu_points.py and tools/points_probe.py share ------------

EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
A = abi.DISPATCH_AUTO
CLR = abi.LIGHTS_COLOR
W, H = MR.SHAPE
N = W * H
OUTS = ("rgba", "ao", "shadow", "material", "steps")
GUARD = 64   # guard rows in front of and behind every output (a wave's worth)


def the_frame(name, pose, prec=EXACT, dispatch=A):
    if name in ("PJ", "PJC"):
        return points_scene(prec, counted=name == "PJC")
    f = scenes.config(name, W, H, precision=prec, pose=pose)
    f.params.dispatch = dispatch
    return f


def mats_of(f, pal=True):
    if f.scene.kind != abi.SCENE_PRIMITIVES:
        return [f.material]
    return scenes.palette(f.scene.count) if pal else [f.material] * f.scene.count


def kernel_shade(rd, f, P, normals=None, eye=None, lift=0.0, lights=None, flags=0,
                 materials=None, outs=OUTS):
    """sdf_shade_points into fenced buffers (gpu_support.fenced) whose GUARD
    rows, in front of every output and behind it, are checked: a RefShade of
    NumPy arrays (None for an output not in `outs`; dif is not an output)."""
    import torch
    dev = lambda a: torch.from_numpy(np.array(a, dtype=f32).reshape(-1, 3)).to(rd.device)
    pts = dev(P)
    n = pts.shape[0]
    nrm = None if normals is None else dev(normals)
    lights = [f.light] if lights is None else list(lights)
    materials = mats_of(f, False) if materials is None else list(materials)
    nl = len(lights)
    larr = (abi.sdf_light * nl)(*lights)
    marr = (abi.sdf_material * len(materials))(*materials)
    shapes = {"rgba": ((n, 4), torch.float32), "ao": ((n,), torch.float32),
              "shadow": ((n, nl), torch.float32), "material": ((n, 9), torch.float32),
              "steps": ((n, nl), torch.int32)}
    mid = {k: fenced(torch, rd.device, *shapes[k], guard=GUARD, front=True) for k in outs}
    p = abi.sdf_points()
    p.points, p.n, p.lift = pts.data_ptr(), n, float(lift)
    p.normals = nrm.data_ptr() if nrm is not None else None
    if eye is not None:
        p.flags = abi.POINTS_EYE
        for c in range(3):
            p.eye[c] = float(eye[c])
    ps = abi.sdf_point_shade(*[mid[k].data_ptr() if k in mid else None for k in OUTS])
    rc = rd.lib.sdf_shade_points(C.byref(f.scene), larr, nl, int(flags), marr, len(materials),
                                 C.byref(f.params), C.byref(p), C.byref(ps), None)
    torch.cuda.synchronize()
    assert rc == abi.SDF_OK, rc
    for k, b in mid.items():
        assert untouched(torch, b), f"{k}: entries in front of the buffer or past its end written"
    got = {k: (mid[k].cpu().numpy() if k in mid else None) for k in OUTS}
    return RefShade(got["rgba"], got["ao"], got["shadow"], got["material"], got["steps"], None)


_HITS = {}


def frame_hits(rd, name, pose):
    """(P (851, 3), eye) of the exact frame: P_0 = O_0 + D_0 d formed on the host
    in unfused fp32 from trace_camera's t and camera_rays, as the render forms
    it."""
    if (name, pose) not in _HITS:
        assert (W, H) == (37, 23) and N == 851 == 13 * 64 + 19
        f = the_frame(name, pose)
        t = rd.trace_camera(f, normal=False, prim=False, steps=False).t
        o, d = rd.camera_rays(f)
        rd.torch.cuda.synchronize()
        o, d, t = o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()
        P = hit_points(o, d, t).reshape(N, 3)
        eye = o.reshape(N, 3)[0].copy()
        assert same(o.reshape(N, 3), np.tile(eye, (N, 1)))
        P.setflags(write=False)
        _HITS[(name, pose)] = (P, eye)
    return _HITS[(name, pose)]


FAST_CASES = [("C4", 0, False), ("C3", 2, True), ("REF", 0, True)]


def fast_deviation(rd, name, pose, pal):
    """The largest absolute deviation of each output of the fast kernel from the
    reference replayed at the kernel's own shadow counts, over all 851 hit
    points under three coloured lights (`material`: where no hard decision of
    the fold is closer than materials_ref.GAP), and how many points that is."""
    f = the_frame(name, pose, FAST)
    mats = mats_of(f, pal)
    P, eye = frame_hits(rd, name, pose)
    got = kernel_shade(rd, f, P, eye=eye, lights=LIGHTS[:3], flags=CLR, materials=mats)
    ref = shade(the_frame(name, pose), P, eye=eye, lights=LIGHTS[:3], light_flags=CLR,
                materials=mats, steps=got.steps)
    assert np.array_equal(ref.steps, np.minimum(got.steps, f.params.max_steps))
    dev = {}
    for k in ("rgba", "ao", "shadow"):
        a, b = getattr(got, k).astype(np.float64), getattr(ref, k).astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        dev[k] = float(np.abs(a - b).max())
    gap = np.array([MR.fold_at(f.scene, mats, *map(float, p))[2] for p in P], dtype=f32)
    far = ~(gap < f32(MR.GAP))
    dev["material"] = float(np.abs(got.material[far].astype(np.float64) -
                                   ref.material[far].astype(np.float64)).max())
    return dev, int(far.sum())
