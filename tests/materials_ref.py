"""Reference of per-primitive materials (include/sdf_abi.h "Materials",
sdf_render_materials) and what its tests share.

The fold itself is C over the CPU oracle (tests/materials_ref.c, compiled on
first use like oracle.load; sdf3d_amd/build.py build_materials_ref builds it
with the rest): at the oracle's own hit point P of every pixel it gives the
blended amb, dif and ref, the scene fold's final d, the primitive that owns
the pixel and `min_gap`, the smallest |a - b| over the hard decisions after
primitive 0 -- a pixel whose min_gap is tiny may flip its owner under another
precision's rounding of P.

compose_px is lights_ref.compose with per-pixel material arrays.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import lights_ref as LR
import oracle
from sdf3d_amd import abi, scenes

f32 = np.float32
HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "build" / "libmaterials_ref.so"
AMB, DIF, REF, POINT, INFO = range(5)
SHAPE = LR.SHAPE
GAP = 1e-3          # hard decisions closer than this are not compared across precisions
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        from sdf3d_amd import build
        build.build_materials_ref(verbose=False)
    lib = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    lib.sdf_materials_ref_render.argtypes = [
        P(abi.sdf_scene), P(abi.sdf_camera), P(abi.sdf_light), P(abi.sdf_material), C.c_int,
        P(abi.sdf_params), P(abi.sdf_tiling), C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.sdf_materials_ref_render.restype = C.c_int
    lib.sdf_materials_ref_fold.argtypes = [
        P(abi.sdf_scene), P(abi.sdf_material), C.c_int, C.c_float, C.c_float, C.c_float,
        C.c_void_p, C.c_void_p]
    lib.sdf_materials_ref_fold.restype = C.c_int
    _lib = lib
    return lib


def marr(materials):
    materials = list(materials)
    return (abi.sdf_material * max(len(materials), 1))(*materials), len(materials)


def plane(frame, materials, what, steps=None):
    """One plane of the reference fold per pixel, [H, W, 4] float32 (`what`:
    AMB / DIF / REF: the blended components and 1; POINT: P and the fold's
    final d; INFO: min_gap, owner, blended, final d).  `steps` ([H, W, 2]):
    the marches are replayed at these counts instead of their own breaks."""
    p = frame.params
    arr, n = marr(materials)
    out = np.full((p.height, p.width, 4), np.nan, dtype=f32)
    force = None
    if steps is not None:
        force = np.ascontiguousarray(np.asarray(steps, dtype=np.int32).reshape(
            p.height, p.width, 2))
    rc = load().sdf_materials_ref_render(
        C.byref(frame.scene), C.byref(frame.camera), C.byref(frame.light), arr, n,
        C.byref(frame.params), None,
        force.ctypes.data_as(C.c_void_p) if force is not None else None, what,
        out.ctypes.data_as(C.c_void_p), oracle.default_threads())
    if rc != 0:
        raise RuntimeError(f"materials reference failed: {rc}")
    return out


def fold(frame, materials, steps=None):
    """The reference fold of every pixel: dict of amb, dif, ref ([H, W, 3]),
    P ([H, W, 3]), d, min_gap ([H, W]), owner (int), blended (bool)."""
    a, d, r = (plane(frame, materials, w, steps)[..., :3].copy() for w in (AMB, DIF, REF))
    pt = plane(frame, materials, POINT, steps)
    info = plane(frame, materials, INFO, steps)
    assert np.array_equal(pt[..., 3].view(np.uint32), info[..., 3].view(np.uint32))
    return {"amb": a, "dif": d, "ref": r, "P": pt[..., :3].copy(), "d": pt[..., 3].copy(),
            "min_gap": info[..., 0].copy(), "owner": info[..., 1].astype(int),
            "blended": info[..., 2] != 0}


def fold_at(scene, materials, x, y, z):
    """The fold at one point: (m[9], d, min_gap, owner, blended, last t)."""
    arr, n = marr(materials)
    m = np.zeros(9, dtype=f32)
    info = np.zeros(5, dtype=f32)
    rc = load().sdf_materials_ref_fold(C.byref(scene), arr, n, float(x), float(y), float(z),
                                       m.ctypes.data_as(C.c_void_p),
                                       info.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return m, f32(info[0]), f32(info[1]), int(info[2]), bool(info[3]), f32(info[4])


def compose_px(frame, terms_list, lights, amb, dif, ref, flags=0,
               precision=abi.PRECISION_EXACT, specs=None):
    """lights_ref.compose with the pixel's own material: amb, dif, ref are
    [rows, W, 3] float32 (the blended components) in place of frame.material's;
    lam[c] = RN(la * amb[c]) per pixel."""
    assert len(terms_list) == len(lights) >= 1
    exact = precision == abi.PRECISION_EXACT
    if specs is None:
        assert exact, "fast precision's spec is the kernel's own: pass `specs`"
        specs = [LR.spec_exact(t[..., 2], frame.material.shininess) for t in terms_list]
    ao = np.asarray(terms_list[0][..., 0], f32)
    la = f32(lights[0].ambient)
    for l in lights[1:]:
        la = f32(la + f32(l.ambient))
    out = np.empty(terms_list[0].shape, dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            lam = (la * np.asarray(amb[..., c], f32)).astype(f32)
            md, mr = np.asarray(dif[..., c], f32), np.asarray(ref[..., c], f32)
            acc = (lam * ao).astype(f32)
            for l, t, sp in zip(lights, terms_list, specs):
                d, s = np.asarray(t[..., 1], f32), np.asarray(sp, f32)
                if flags & abi.LIGHTS_COLOR:
                    col = f32(l.color[c])
                    d, s = (d * col).astype(f32), (s * col).astype(f32)
                if exact:
                    acc = (acc + (d * md).astype(f32)).astype(f32)
                    acc = (acc + (s * mr).astype(f32)).astype(f32)
                else:
                    acc = LR.fma32(s, mr, LR.fma32(d, md, acc))
            out[..., c] = acc
    out[..., 3] = f32(1.0)
    return out


def constant(frame, m):
    """(amb, dif, ref) arrays holding material `m` on every pixel."""
    shape = (frame.params.height, frame.params.width, 3)
    return tuple(np.broadcast_to(np.array([f32(v[c]) for c in range(3)], dtype=f32), shape)
                 for v in (m.amb, m.dif, m.ref))


# ---- the SIX test scenes: all six operators, all seven kinds --------------------

def six(precision=abi.PRECISION_EXACT, hard_last=False, wh=SHAPE):
    """config C3, pose 2, with seven primitives that use every kind and every
    operator; `hard_last`: primitive 6 is a BOX in hard INTERSECT instead of a
    SPHERE in SMOOTH_INTERSECT."""
    f = scenes.config("C3", *wh, precision=precision, pose=2)
    s = f.scene
    C.memset(C.addressof(s.prims), 0, C.sizeof(s.prims))
    s.count = 7
    P = scenes._prim
    P(s, 0, abi.PRIM_PLANE, abi.OP_UNION, 0.0, 0.0, 1.0, 0.0, 0.0)
    P(s, 1, abi.PRIM_ROUND_BOX, abi.OP_UNION, 0.0, 0.0, 0.3, 0.0, 0.3, 0.3, 0.3, 0.05)
    P(s, 2, abi.PRIM_SPHERE, abi.OP_SUBTRACT, 0.0, 0.3, 0.6, 0.3, 0.25)
    P(s, 3, abi.PRIM_TORUS, abi.OP_SMOOTH_UNION, 0.1, -0.6, 0.1, 0.2, 0.2, 0.06)
    P(s, 4, abi.PRIM_CYLINDER, abi.OP_SMOOTH_SUBTRACT, 0.05, -0.2, 0.45, 0.3, 0.08, 0.3)
    P(s, 5, abi.PRIM_CAPSULE, abi.OP_SMOOTH_UNION, 0.08, 0.5, 0.1, 0.4, 0.8, 0.3, 0.1, 0.07)
    if hard_last:
        P(s, 6, abi.PRIM_BOX, abi.OP_INTERSECT, 0.0, 0.0, 0.0, 0.0, 1.5, 1.5, 1.5)
    else:
        P(s, 6, abi.PRIM_SPHERE, abi.OP_SMOOTH_INTERSECT, 0.1, 0.0, 0.0, 0.0, 1.6)
    f.name = "SIXH" if hard_last else "SIX"
    return f


def frame_of(name, pose=0, precision=abi.PRECISION_EXACT, wh=SHAPE):
    """REF / C2 / C3 / C4 at `pose`, or SIX / SIXH (their own pose)."""
    if name in ("SIX", "SIXH"):
        return six(precision, name == "SIXH", wh)
    return scenes.config(name, *wh, precision=precision, pose=pose)


FRAMES = [("REF", 0), ("C2", 1), ("C3", 2), ("C4", 0), ("SIX", 2), ("SIXH", 2)]


def palette_for(frame):
    return scenes.palette(frame.scene.count)
