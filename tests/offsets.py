"""Translated scenes: a whole frame moved by a vector T without being scaled,
and what the tests of culling far from the origin share.  TEST INFRASTRUCTURE
ONLY.

A unit-size scene at coordinates of magnitude M is where the culling margins
are hardest to hold: the fp32 spacing of the coordinates grows with M (ulp(1e4)
is 9.8e-4) while every radius, blend radius and the absolute margin kCullAbs =
1e-4 stay what they were.  tools/scale_exactness_probe.py scales the sizes with
the coordinates; this module does not.

  translate(frame, T)   the frame moved by T: primitives, light, camera
  OFFSETS               the named offsets the tests use
  far(bound, P, d)      the kernels' culling test (render_kernel.inc wave_near),
                        restated in NumPy fp32
  pair_scene(...)       a (competitor, primitive) scene and probe points on and
                        just outside the primitive's bounding shell, where the
                        bounding sphere is tight and the competitor's value
                        sweeps across the primitive's
  csg8_probe(...)       the same inside a scene of the CSG8 signature, which
                        the built-in fixed kernel runs
  case_frame, coverage  the frames of tests/test_gpu_offsets.py and the share
                        of their pixels that shows a cullable primitive
"""
import ctypes as C

import numpy as np

import fast_paths as FP
import oracle
from cases import random_csg8
from sdf3d_amd import abi

f32 = np.float32
REL = f32(1e-5)                                 # kernel_args.h kCullRel
SCALE = f32(1.0) / (f32(1.0) - REL)             # kCullScale

# The offsets: magnitude m times a direction, with m no multiple of a large
# power of two, so that midpoints and centres really round.
MAGNITUDES = {"1e3": 1000.7, "1e4": 10007.3, "1e5": 100003.7, "2^20": 2.0 ** 20 + 3.3}
DIRECTIONS = {"xz": (1.0, 0.0, 1.0), "skew": (-1.0, 0.3, 0.7), "z": (0.0, 0.0, 1.0)}
OFFSETS = {"0": np.zeros(3)}
for _m, _mag in MAGNITUDES.items():
    for _d, _dir in DIRECTIONS.items():
        OFFSETS[f"{_m}-{_d}"] = _mag * np.array(_dir, dtype=np.float64)
MOVED = [k for k in OFFSETS if k != "0"]


def magnitude(name):
    return float(np.abs(OFFSETS[name]).max())


def _moved(v, t):
    """fp32 v moved by t in float64, rounded once; untouched where t is 0."""
    return float(v) if t == 0.0 else float(f32(np.float64(v) + np.float64(t)))


def translate_scene(scene, T):
    """A copy of `scene` with every position parameter moved by T: centres,
    both end points of a capsule, a plane's offset by -n.T, the Mandelbulb's
    centre.  Sizes and blend radii stay."""
    T = np.asarray(T, dtype=np.float64)
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(scene), C.sizeof(s))
    for i in range(s.count if s.kind == abi.SCENE_PRIMITIVES else 0):
        pr = s.prims[i]
        if pr.kind == abi.PRIM_PLANE:
            n = np.array([pr.p[0], pr.p[1], pr.p[2]], dtype=np.float64)
            pr.p[3] = _moved(pr.p[3], -float(n @ T))
            continue
        for j in range(3):
            pr.p[j] = _moved(pr.p[j], T[j])
        if pr.kind == abi.PRIM_CAPSULE:
            for j in range(3):
                pr.p[3 + j] = _moved(pr.p[3 + j], T[j])
    for j in range(3):
        s.bulb_center[j] = _moved(s.bulb_center[j], T[j])
    return s


def translate(frame, T):
    """`frame` moved by T.  The view matrix is composed with the translation
    in float64 and rounded once (V' = V . translate(-T): only its fourth column
    changes, so inverse(V') eye = inverse(V) eye + T); eps, normal_eps, the AO
    heights and max_dist stay.  T = 0 gives the frame's own bits."""
    T = np.asarray(T, dtype=np.float64)
    g = frame.copy()
    g.scene = translate_scene(frame.scene, T)
    for j in range(3):
        g.light.pos[j] = _moved(frame.light.pos[j], T[j])
    if np.any(T != 0.0):
        V = np.array(list(frame.camera.view), dtype=np.float64).reshape(4, 4).T   # column-major
        col = V[:, 3] - V[:, :3] @ T
        for r in range(4):
            g.camera.view[12 + r] = float(f32(col[r]))
    g.meta["offset"] = [float(t) for t in T]
    return g


def same_bytes(a, b):
    return bytes(a) == bytes(b)


# ---- the culling test, restated ---------------------------------------------
def far(bound, P, d):
    """Where the kernels' test (wave_near) calls the points P far from the
    bound (cx, cy, cz, K') at accumulator d: dd >= T T with T = fma(d,
    kCullScale, K') and dd = |p - c|^2 in fp32.  The kernels form dd fused
    (two FMAs) or, for a sphere's own bound, as the plain sum; a point is
    reported far when either reading says so, the more demanding claim."""
    b = np.asarray(bound, dtype=f32)
    P = np.asarray(P, dtype=f32)
    d = np.asarray(d, dtype=f32)
    with np.errstate(all="ignore"):
        v = P - b[:3]                                          # fp32 subtractions
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        plain = (x * x + y * y) + z * z
        zz = (z * z).astype(np.float64)
        inner = (y.astype(np.float64) * y + zz).astype(f32).astype(np.float64)
        fused = (x.astype(np.float64) * x + inner).astype(f32)
        T = (d.astype(np.float64) * np.float64(SCALE) + np.float64(b[3])).astype(f32)
        TT = T * T
        return (plain >= TT) | (fused >= TT)


def bounds_of(scene):
    """(rc, bounds (16, 4) float32, cluster (4,) float32, cluster_first) of
    sdf_scene_bounds."""
    lib = abi.load_library()
    b = (C.c_float * (4 * abi.SDF_MAX_PRIMS))()
    c = (C.c_float * 4)()
    first = C.c_int32()
    rc = lib.sdf_scene_bounds(C.byref(scene), b, c, C.byref(first))
    return rc, np.array(b, dtype=f32).reshape(-1, 4), np.array(c, dtype=f32), first.value


def sdf_at(scene, P):
    return np.array([oracle.scene_sdf(scene, float(p[0]), float(p[1]), float(p[2])) for p in P],
                    dtype=f32)


def cut(scene, n):
    """The first n primitives of `scene`."""
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(scene), C.sizeof(s))
    s.count = n
    return s


CULL_PATH = 2.0 ** -20      # sdf_abi.cpp kCullPath
CULL_REL = 1e-5             # kernel_args.h kCullRel


def plan_bound(bound, reach):
    """(lo, hi): the bound a gap-caching plan (SDF_DISPATCH_AUTO, ray segments
    up to `reach` = max_dist) reads in place of sdf_scene_bounds' (cx, cy, cz,
    K'), bracketed: sdf_abi.cpp prepare_bounds adds kCullPath (|c|_inf + R + k
    + reach) to the absolute margin, and |c|_inf <= |c|_inf + R + k <= |c|_inf
    + K'.  The test compares |p - c|^2 with T^2, T = d kCullScale + K', whose
    largest value over an interval of K' is taken at an end: a point far by
    both ends is far by the plan's bound."""
    b = np.array(bound, dtype=np.float64)
    cmax = np.abs(b[:3]).max()
    out = []
    for extra, slack in ((0.0, 1.0 - 3e-6), (b[3], 1.0 + 3e-6)):
        v = b.copy()
        v[3] = (b[3] + CULL_PATH * (cmax + extra + reach) / (1.0 - CULL_REL)) * slack
        out.append(v.astype(f32))
    return out[0], out[1]


def says_far(scene, i, P, reach=None):
    """Where the culling of primitive i of `scene` -- the cluster test, then
    the primitive's own -- skips it at the points P, by the restated test on
    sdf_scene_bounds' values alone: the bounds of the generic kernel, which
    makes every test afresh.  With `reach` the bounds are enlarged to what a
    gap-caching plan with that max_dist reads (plan_bound, far by both ends of
    its bracket): the fixed and the run-time specialised kernels' test.  The accumulator before primitive i is
    the oracle's value of the scene cut to its first i primitives; it is the
    accumulator of the cluster test as well when i is the first culled one.
    Returns (far, d)."""
    rc, b, cl, first = bounds_of(scene)
    assert rc == 0 and first <= i < scene.count, (rc, first, i)
    d = sdf_at(cut(scene, i), P)
    if reach is not None:
        res = far(plan_bound(b[i], reach)[0], P, d) & far(plan_bound(b[i], reach)[1], P, d)
        if i == first:
            res |= far(plan_bound(cl, reach)[0], P, d) & far(plan_bound(cl, reach)[1], P, d)
        return res, d
    res = far(b[i], P, d)
    if i == first:
        res |= far(cl, P, d)
    return res, d


# ---- adversarial points: the bounding shell ------------------------------------
CULLABLE = [(kind, op) for kind in (abi.PRIM_SPHERE, abi.PRIM_BOX, abi.PRIM_ROUND_BOX,
                                    abi.PRIM_TORUS, abi.PRIM_CAPSULE, abi.PRIM_CYLINDER)
            for op in (abi.OP_UNION, abi.OP_SMOOTH_UNION)
            if not (kind == abi.PRIM_SPHERE and op == abi.OP_UNION)]   # kernel_args.h cullable()
SWEEP = 2e-3          # the competitor's value sweeps this far either side of the primitive's


def random_primitive(rng, kind, op, pr):
    """Unit-size parameters of `kind` about the origin into `pr`."""
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    C.memset(C.addressof(pr), 0, C.sizeof(pr))
    pr.kind, pr.op = kind, op
    pr.k = u(0.02, 0.15) if op == abi.OP_SMOOTH_UNION else 0.0
    for j in range(3):
        pr.p[j] = u(-1, 1)
    if kind == abi.PRIM_SPHERE:
        pr.p[3] = u(0.05, 0.4)
    elif kind in (abi.PRIM_BOX, abi.PRIM_ROUND_BOX):
        for j in range(3, 6):
            pr.p[j] = u(0.05, 0.4)
        if kind == abi.PRIM_ROUND_BOX:
            pr.p[6] = u(0.1, 0.8) * min(pr.p[3], pr.p[4], pr.p[5])
    elif kind == abi.PRIM_TORUS:
        pr.p[3], pr.p[4] = u(0.1, 0.4), u(0.02, 0.1)
    elif kind == abi.PRIM_CAPSULE:
        for j in range(3, 6):
            pr.p[j] = u(-1, 1)
        pr.p[6] = u(0.02, 0.3)
    elif kind == abi.PRIM_CYLINDER:
        pr.p[3], pr.p[4] = u(0.05, 0.3), u(0.05, 0.4)


def farthest(pr, rng):
    """(F, rho, U, D): a direction U in which the primitive reaches its
    bounding sphere, the centre F and radius rho of the feature it ends in
    there -- beyond it, near U, the primitive's value is |p - F| - rho (exactly
    for a capsule's cap, a sphere, a box's corner; to second order for the rims
    of a torus and a cylinder) -- and the distance D of F from the bounding
    sphere's centre.  float64, from the fp32 parameters."""
    p = np.array(list(pr.p), dtype=np.float64)
    c = p[0:3]
    sg = rng.choice([-1.0, 1.0], size=3)
    phi = rng.uniform(0, 2 * np.pi)
    ring = np.array([np.cos(phi), 0.0, np.sin(phi)])
    if pr.kind == abi.PRIM_SPHERE:
        U = rng.normal(size=3)
        return c, p[3], U / np.linalg.norm(U), 0.0
    if pr.kind == abi.PRIM_BOX:
        e = sg * p[3:6]
    elif pr.kind == abi.PRIM_ROUND_BOX:
        e = sg * np.maximum(p[3:6] - p[6], 0.0)
    elif pr.kind == abi.PRIM_TORUS:
        e = p[3] * ring
    elif pr.kind == abi.PRIM_CAPSULE:
        a, b = p[0:3], p[3:6]
        if sg[0] < 0:
            a, b = b, a
        c, e = 0.5 * (a + b), 0.5 * (b - a)
    else:
        assert pr.kind == abi.PRIM_CYLINDER
        e = p[3] * ring + np.array([0.0, sg[1] * p[4], 0.0])
    rho = {abi.PRIM_ROUND_BOX: abs(p[6]), abi.PRIM_TORUS: p[4],
           abi.PRIM_CAPSULE: p[6]}.get(pr.kind, 0.0)
    D = float(np.linalg.norm(e))
    return c + e, rho, e / D, D


def cone_points(rng, F, rho, U, n, w, top, reach=1.0):
    """n fp32 points beyond the feature (F, rho) in a cone about U, at
    distances t = rho + [0, reach] from F.  The value of a sphere about
    F - w U falls behind the feature's own by t w / (t + w) (1 - cos) at the
    angle off U; the angles are drawn so that this loss is uniform in [0, top
    + SWEEP].  Duplicates (coarse coordinates) are dropped."""
    a = np.cross(U, [1.0, 0.0, 0.0] if abs(U[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(U, a)
    t = rho + rng.uniform(1e-3, reach, n)
    cos = np.maximum(1.0 - rng.uniform(0.0, top + SWEEP, n) * (t + w) / (t * w), -1.0)
    sin = np.sqrt(np.maximum(1.0 - cos * cos, 0.0))
    psi = rng.uniform(0, 2 * np.pi, n)
    e = cos[:, None] * U + sin[:, None] * (np.cos(psi)[:, None] * a + np.sin(psi)[:, None] * b)
    P = (F + t[:, None] * e).astype(f32)
    return np.unique(P, axis=0)


def sphere_competitor(pr, F, rho, U, D, ulp, top, comp):
    """The competitor into `comp`: a hard-union sphere about q = F - w U (fp32)
    whose value, on the ray from q through F, exceeds the primitive's by
    `top` (hard union) or by top - k (smooth union); off the ray it falls
    behind, and so does the bounding sphere's gap, but by D / w as much: w is
    40 D, at least 0.05 and two coordinate spacings.  Returns w."""
    w = max(40.0 * D, 0.05, 2.0 * ulp)
    q = (F - w * U).astype(f32)
    k = pr.k if pr.op == abi.OP_SMOOTH_UNION else 0.0
    radius = np.linalg.norm(F - q.astype(np.float64)) + rho + k - top
    C.memset(C.addressof(comp), 0, C.sizeof(comp))
    comp.kind, comp.op = abi.PRIM_SPHERE, abi.OP_UNION
    for j in range(3):
        comp.p[j] = float(q[j])
    comp.p[3] = float(f32(radius))
    return w


def pair_scene(template, T, rng, kind, op, n=700):
    """A two-primitive scene [competitor, primitive] at offset T and the probe
    points of one of the primitive's farthest directions.  Returns (scene, P)."""
    T = np.asarray(T, dtype=np.float64)
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(template), C.sizeof(s))
    C.memset(C.addressof(s.prims), 0, C.sizeof(s.prims))
    s.kind, s.count = abi.SCENE_PRIMITIVES, 2
    random_primitive(rng, kind, op, s.prims[1])
    s = translate_scene(s, T)
    pr = s.prims[1]
    F, rho, U, D = farthest(pr, rng)
    ulp = float(np.spacing(f32(np.abs(T).max())))
    # the sweep's upper end: +SWEEP, or closer to the value at which the
    # primitive starts to matter, where the points near the ray are the probes
    top = SWEEP * float(rng.choice([1.0, 0.25, 0.05]))
    w = sphere_competitor(pr, F, rho, U, D, ulp, top, s.prims[0])
    return s, cone_points(rng, F, rho, U, n, w, top)


def single(scene, i):
    """Primitive i of `scene` alone, as a hard union."""
    s = cut(scene, 1)
    C.memmove(C.addressof(s.prims[0]), C.addressof(scene.prims[i]), C.sizeof(abi.sdf_primitive))
    s.prims[0].op = abi.OP_UNION
    return s


def in_sweep(scene, i, P, d):
    """The points at which the accumulator d before primitive i lies within
    SWEEP of the value at which the primitive starts to matter: |d - s| (hard
    union) or |d + k - s| (smooth union) <= SWEEP, by the oracle's values."""
    pr = scene.prims[i]
    s = sdf_at(single(scene, i), P).astype(np.float64)
    k = pr.k if pr.op == abi.OP_SMOOTH_UNION else 0.0
    return np.abs(d.astype(np.float64) + k - s) <= SWEEP


# ---- the frames of the GPU tests ----------------------------------------------------
WH = (96, 54)
RENDER_CASES = ["C4-p0", "C4-p1", "csg8-1", "csg8-4", "C4-generic", "C4-carved", "materials",
                "reflect"]


def base_frame(case, wh=WH):
    """The untranslated frame of a render case, exact precision."""
    if case.startswith("csg8-"):
        seed = int(case.split("-")[1])
        f = random_csg8(np.random.default_rng(seed), [0.5, 1.0, 2.5][seed % 3],
                        [0.05, 0.3, 1.0][(seed // 3) % 3])
        f.params.width, f.params.height = wh
    elif case == "C4-carved":
        f = FP.PATHS[case](abi.PRECISION_EXACT, wh)
    else:
        from sdf3d_amd import scenes
        pose = {"C4-p1": 1, "materials": 2}.get(case, 0)
        f = scenes.config("C4", *wh, pose=pose)
        if case == "C4-generic":
            f.params.dispatch = abi.DISPATCH_GENERIC
    f.params.precision = abi.PRECISION_EXACT
    return f


def case_frame(case, name, wh=WH):
    """The frame of `case` at offset `name`.  (No eye has to move closer: at
    2^20, with 8 representable positions per unit, the frames show more of the
    primitives than at the origin -- coverage().)"""
    return translate(base_frame(case, wh), OFFSETS[name])


def coverage(frame):
    """By the oracle alone: the share of the frame's pixels whose primary march
    ends on the surface (below eps, within max_dist) of a cullable primitive
    (the oracle's owner fold at the hit point)."""
    import query_ref as Q
    O_, D = Q.camera_rays(frame)
    t, _ = Q.march(frame, O_, D)
    hit = ~(t > f32(frame.params.max_dist))
    idx = np.nonzero(hit)[0]
    own, _ = Q.owner(frame, Q.point(O_[idx], D[idx], t[idx]))
    sc = frame.scene
    cullable = np.array([sc.prims[i].kind != abi.PRIM_PLANE and
                         (sc.prims[i].op == abi.OP_SMOOTH_UNION or
                          (sc.prims[i].op == abi.OP_UNION and sc.prims[i].kind != abi.PRIM_SPHERE))
                         for i in range(sc.count)])
    return float(cullable[own].sum()) / len(t)


# ---- probes on the fixed CSG8 kernel ---------------------------------------------------
CSG8_PROBED = {"capsule": 4, "box": 2, "sphere": 7}   # set_csg8's indices
PARKED = 30.0


def plan_margin(T, reach):
    """What a gap-caching plan with max_dist `reach` adds to the absolute
    margin of a unit-size primitive at offset T (prepare_bounds: kCullPath
    (|c|_inf + R + k + reach)), to within the primitive's own size."""
    return CULL_PATH * (float(np.abs(np.asarray(T, dtype=np.float64)).max()) + 2.0 + reach)


def csg8_probe(template, T, rng, which, n=700, reach=None):
    """A scene with the CSG8 signature (the built-in fixed kernel runs it) in
    which primitive `which` meets the head plane alone: the other six are
    parked PARKED away, where no smooth union feels them, and the plane y = h
    is the competitor.  Its normal is +y, so the primitive stands upright -- a
    near-vertical capsule, a thin tall box, a sphere -- and the probe points
    lie in the cone above its top, where the plane's value sweeps across the
    primitive's (cone_points with the competitor's centre infinitely far
    below).  With `reach` (the max_dist of the plan that will run the scene)
    the plane is lowered by up to 1.5 times the margin a gap-caching plan adds
    at this offset (plan_margin: 0.01 at 1e4, 1.0 at 2^20), so that the sweep
    crosses the value at which that plan's enlarged bounds call the primitive
    far, not the generic kernel's alone.  Returns (scene, P, i)."""
    from sdf3d_amd import scenes
    T = np.asarray(T, dtype=np.float64)
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(template), C.sizeof(s))
    scenes.set_csg8(s)
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    for i in range(1, 8):
        ang = 2 * np.pi * i / 7
        dx, dz = PARKED * np.cos(ang) - s.prims[i].p[0], PARKED * np.sin(ang) - s.prims[i].p[2]
        s.prims[i].p[0] += dx
        s.prims[i].p[2] += dz
        if s.prims[i].kind == abi.PRIM_CAPSULE:
            s.prims[i].p[3] += dx
            s.prims[i].p[5] += dz
    i = CSG8_PROBED[which]
    pr = s.prims[i]
    pr.k = u(0.02, 0.1)
    x, y, z = u(-0.5, 0.5), u(0.2, 0.6), u(-0.5, 0.5)
    if which == "capsule":
        half = u(0.05, 0.15)
        pr.p[0], pr.p[1], pr.p[2] = x, y, z
        pr.p[3], pr.p[4], pr.p[5] = x + u(-0.004, 0.004), y + 2 * half, z + u(-0.004, 0.004)
        pr.p[6] = u(0.03, 0.12)
    elif which == "box":
        pr.p[0], pr.p[1], pr.p[2] = x, y, z
        pr.p[3], pr.p[4], pr.p[5] = u(0.004, 0.01), u(0.15, 0.3), u(0.004, 0.01)
    else:
        pr.p[0], pr.p[1], pr.p[2], pr.p[3] = x, y, z, u(0.05, 0.3)
    s = translate_scene(s, T)
    pr = s.prims[i]
    p = np.array(list(pr.p), dtype=np.float64)
    up = np.array([0.0, 1.0, 0.0])
    if which == "capsule":
        F, rho = p[3:6], p[6]
    elif which == "box":
        F, rho = p[0:3] + p[3:6] * np.sign(rng.uniform(-1, 1, 3)) * [1, 0, 1] + [0, p[4], 0], 0.0
    else:
        F, rho = p[0:3], p[3]
    top = SWEEP * float(rng.choice([1.0, 0.25, 0.05]))
    shift = 0.0 if reach is None else float(rng.uniform(0.0, 1.5)) * plan_margin(T, reach)
    # on the ray above F: plane = p.y + h, primitive = p.y - F.y - rho
    s.prims[0].p[3] = float(f32(top - shift - pr.k - F[1] - rho))
    return s, cone_points(rng, F, rho, up, n, 1e9, top), i
