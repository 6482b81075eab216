"""Reference of mirror reflections (include/sdf_abi.h "Reflections",
sdf_render_reflect) and what its tests share.

The path itself is walked in C over the CPU oracle (tests/reflect_ref.c,
compiled on first use; sdf3d_amd/build.py build_reflect_ref builds it with the
rest): per pixel and layer j it records the eye and ray (O, D), the oracle's
own P, N, d, ao and step counts for that fragment, every light's (dif_i, x_i),
and the blended amb, dif and ref at P.  This module states the rest in NumPy,
fp32 round to nearest, never reassociated:

    C_j              materials_ref.compose_px of layer j's terms and materials
    W_0 = 1          k_j[c] = RN(strength ref_j[c]),  W_(j+1)[c] = RN(W_j[c] k_j[c])
    composite        acc = C_0;  j = 1 .. last in order
                       exact   acc = RN(acc + RN(W_j C_j))
                       fast    acc = fma(W_j, C_j, acc)
    steps            (sum_j primary_j, sum_j sum_i shadow_(j, i))

A layer the path did not reach contributes nothing (its planes are zero and
`alive` is False).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import lights_ref as LR
import materials_ref as MR
import oracle
from sdf3d_amd import abi

f32 = np.float32
HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "build" / "libreflect_ref.so"
SHAPE = MR.SHAPE
# tests/reflect_ref.c RF_*
ALIVE, O_, D_, P_, N_, DIST, AO, MAT, W_, SP, SS, DIF, X_, OWN, FLOATS = (
    0, 1, 4, 7, 10, 13, 14, 15, 24, 27, 28, 36, 44, 52, 56)
FORCE = 1 + abi.MAX_LIGHTS
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        from sdf3d_amd import build
        build.build_reflect_ref(verbose=False)
    MR.load()   # libmaterials_ref.so: the fold this library links against
    lib = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    lib.sdf_reflect_ref_render.argtypes = [
        P(abi.sdf_scene), P(abi.sdf_camera), P(abi.sdf_light), C.c_int, P(abi.sdf_material),
        C.c_int, C.c_int, C.c_float, P(abi.sdf_params), P(abi.sdf_tiling), C.c_void_p,
        C.c_void_p, C.c_int]
    lib.sdf_reflect_ref_render.restype = C.c_int
    lib.sdf_reflect_ref_floats.restype = C.c_int
    assert lib.sdf_reflect_ref_floats() == FLOATS
    _lib = lib
    return lib


def materials_for(frame, materials=None):
    """`materials`, or frame.material once per primitive (one for a Mandelbulb)."""
    if materials is not None:
        return list(materials)
    prims = frame.scene.kind == abi.SCENE_PRIMITIVES
    return [frame.material] * (frame.scene.count if prims else 1)


def walk(frame, materials, bounces, strength, lights=None, force=None):
    """Every pixel's path as the C reference walks it: dict of
    alive [H, W, J] bool (J = bounces + 1); O, D, P, N, amb, dif, ref, W, own
    [H, W, J, 3]; d, ao [H, W, J]; sp [H, W, J] and ss [H, W, J, L] int;
    difs, xs [H, W, J, L].  `force` ([H, W, J, 1 + MAX_LIGHTS] int: primary,
    light i's shadow): step counts imposed on the layers the reference reaches."""
    p = frame.params
    lights = [frame.light] if lights is None else list(lights)
    L = len(lights)
    larr = (abi.sdf_light * L)(*lights)
    marr, n = MR.marr(materials_for(frame, materials))
    J = bounces + 1
    out = np.zeros((p.height, p.width, J, FLOATS), dtype=f32)
    fo = None
    if force is not None:
        fo = np.ascontiguousarray(np.asarray(force, dtype=np.int32).reshape(
            p.height, p.width, J, FORCE))
    rc = load().sdf_reflect_ref_render(
        C.byref(frame.scene), C.byref(frame.camera), larr, L, marr, n, int(bounces),
        C.c_float(strength), C.byref(frame.params), None,
        fo.ctypes.data_as(C.c_void_p) if fo is not None else None,
        out.ctypes.data_as(C.c_void_p), oracle.default_threads())
    if rc != 0:
        raise RuntimeError(f"reflect reference failed: {rc}")
    v3 = lambda k: out[..., k:k + 3].copy()
    return {"alive": out[..., ALIVE] != 0, "O": v3(O_), "D": v3(D_), "P": v3(P_), "N": v3(N_),
            "d": out[..., DIST].copy(), "ao": out[..., AO].copy(), "amb": v3(MAT),
            "dif": v3(MAT + 3), "ref": v3(MAT + 6), "W": v3(W_), "own": v3(OWN),
            "sp": out[..., SP].astype(np.int32), "ss": out[..., SS:SS + L].astype(np.int32),
            "difs": out[..., DIF:DIF + L].copy(), "xs": out[..., X_:X_ + L].copy(),
            "lights": lights, "bounces": bounces, "strength": f32(strength)}


def weights(ref, alive, strength):
    """W_j [H, W, J, 3] from the layers' blended ref: W_0 = 1, W_(j+1) =
    RN(W_j RN(strength ref_j)); zero where the path did not reach layer j."""
    Wt = np.zeros(ref.shape, dtype=f32)
    Wt[:, :, 0] = f32(1.0)
    with np.errstate(all="ignore"):
        for j in range(ref.shape[2] - 1):
            k = (f32(strength) * ref[:, :, j]).astype(f32)
            Wt[:, :, j + 1] = (Wt[:, :, j] * k).astype(f32)
    return np.where(alive[..., None], Wt, f32(0.0)).astype(f32)


def layer_colours(frame, w, flags=0):
    """C_j [H, W, J, 3] of a walk, exact precision's operation sequence: the
    "Materials" colour sum of layer j's terms; zero where the path ended."""
    H, Wd, J = w["alive"].shape
    one = np.ones((H, Wd), dtype=f32)
    out = np.zeros((H, Wd, J, 3), dtype=f32)
    for j in range(J):
        terms = [np.stack([w["ao"][:, :, j], w["difs"][:, :, j, i], w["xs"][:, :, j, i], one],
                          axis=-1) for i in range(len(w["lights"]))]
        c = MR.compose_px(frame, terms, w["lights"], w["amb"][:, :, j], w["dif"][:, :, j],
                          w["ref"][:, :, j], flags=flags)
        out[:, :, j] = np.where(w["alive"][:, :, j, None], c[..., :3], f32(0.0))
    return out


def composite(Cj, Wj, alive, precision=abi.PRECISION_EXACT):
    """The composite [H, W, 4] of the layers' colours and weights, in the
    precision's operation sequence, layers in order."""
    acc = np.asarray(Cj[:, :, 0], f32).copy()
    with np.errstate(all="ignore"):
        for j in range(1, Cj.shape[2]):
            if precision == abi.PRECISION_EXACT:
                new = (acc + (Wj[:, :, j] * Cj[:, :, j]).astype(f32)).astype(f32)
            else:
                new = LR.fma32(Wj[:, :, j], Cj[:, :, j], acc)
            acc = np.where(alive[:, :, j, None], new, acc).astype(f32)
    out = np.empty(acc.shape[:2] + (4,), dtype=f32)
    out[..., :3] = acc
    out[..., 3] = f32(1.0)
    return out


def layer_steps(w):
    """[H, W, J, 2] int32: every layer's (primary, summed shadow) counts."""
    return np.stack([w["sp"], w["ss"].sum(axis=-1)], axis=-1).astype(np.int32)


def render(frame, materials, bounces, strength, lights=None, flags=0, force=None):
    """The reference frame: (rgba [H, W, 4], steps [H, W, 2], the walk with its
    layer colours under "C")."""
    w = walk(frame, materials, bounces, strength, lights, force)
    w["C"] = layer_colours(frame, w, flags)
    rgba = composite(w["C"], w["W"], w["alive"])
    return rgba, layer_steps(w).sum(axis=2).astype(np.int32), w


def reflect(bounces, strength, layer=-1, flags=0):
    return abi.sdf_reflect(int(bounces), float(strength), int(layer), int(flags))
