"""The containment the host-side culling bounds must have (sdf_scene_bounds; no
GPU): each kind's bounding sphere restated independently of the library, and the
check that every primitive lies inside its own sphere and every cullable one
inside the cluster sphere.  TEST INFRASTRUCTURE ONLY: what tests/test_bounds.py
and tests/test_offsets.py share."""
import ctypes as C

import numpy as np

from sdf3d_amd import abi

ABS, REL = float(np.float32(1e-4)), float(np.float32(1e-5))   # kCullAbs, kCullRel
SMOOTH = (abi.OP_SMOOTH_UNION,)


def bounds_of(scene):
    lib = abi.load_library()
    b = (C.c_float * (4 * abi.SDF_MAX_PRIMS))()
    c = (C.c_float * 4)()
    first = C.c_int32()
    rc = lib.sdf_scene_bounds(C.byref(scene), b, c, C.byref(first))
    return rc, np.array(b, dtype=np.float64).reshape(-1, 4), np.array(c, dtype=np.float64), first.value


def sphere_of(pr):
    """Centre and radius of a sphere containing the primitive (its own
    statement of the shapes in render_kernel.inc)."""
    p = np.array(pr.p, dtype=np.float64)
    c = p[0:3].copy()
    if pr.kind == abi.PRIM_SPHERE:
        r = p[3]
    elif pr.kind == abi.PRIM_BOX:
        r = np.linalg.norm(p[3:6])
    elif pr.kind == abi.PRIM_ROUND_BOX:       # the box b - r rounded by r
        r = np.linalg.norm(np.maximum(p[3:6] - p[6], 0.0)) + abs(p[6])
    elif pr.kind == abi.PRIM_TORUS:
        r = p[3] + p[4]
    elif pr.kind == abi.PRIM_CAPSULE:
        c = 0.5 * (p[0:3] + p[3:6])
        r = 0.5 * np.linalg.norm(p[3:6] - p[0:3]) + p[6]
    elif pr.kind == abi.PRIM_CYLINDER:
        r = np.hypot(p[3], p[4])
    else:
        r = 0.0
    return c, abs(r)


def check_containment(scene):
    rc, b, cl, first = bounds_of(scene)
    assert rc == 0
    n = scene.count
    centres, radii, ks = [], [], []
    for i in range(n):
        pr = scene.prims[i]
        c, r = sphere_of(pr)
        k = pr.k if pr.op in SMOOTH else 0.0
        if i >= first:
            # containment as the kernel reads it: the sphere of radius
            # K'(1 - rel) - abs - k about the fp32 centre it is handed holds the
            # primitive's true sphere (float64, from the fp32 parameters).  No
            # tolerance: none may grow with |c|, where the centre's rounding
            # does (a capsule's midpoint at |c| = 1e4 is up to 8.5e-4 off)
            held = b[i, 3] * (1 - REL) - ABS - k
            assert np.linalg.norm(b[i, :3] - c) + r <= held, \
                (i, pr.kind, np.linalg.norm(b[i, :3] - c), r, held)
            centres.append(c)
            radii.append(r)
            ks.append(k)
    if first >= n:
        return None
    centres, radii = np.array(centres), np.array(radii)
    kmax = max(ks)
    rc_cluster = cl[3] * (1 - REL) - ABS - kmax   # the radius the cluster bound encloses
    far = np.linalg.norm(centres - cl[:3], axis=1) + radii
    assert np.all(far <= rc_cluster), (far.max(), rc_cluster)      # no tolerance here either
    centroid = centres.mean(axis=0)
    rc_centroid = (np.linalg.norm(centres - centroid, axis=1) + radii).max()
    return rc_cluster, rc_centroid
