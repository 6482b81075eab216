"""The scenes, frames and views that more than one test module uses, and every
scene whose run-time compilations a test counts.  TEST INFRASTRUCTURE ONLY;
CPU only (no torch, no test module).

A scene whose (kind, op) sequence matches no built-in variant is compiled at run
time (hipRTC) under SDF_DISPATCH_AUTO, once per process and kernel family.  A
test that counts those compilations passes only if no other test of the process
renders that sequence first.  COUNTED lists every such scene; the run-time
specialised scenes the tests use without counting are in UNCOUNTED, and
tests/test_gpu_support_ref.py holds all of them apart from one another and from
the built-in variants."""
import ctypes as C

import numpy as np

import env_ref as ER
import lights_ref as LR
import materials_ref as MR
import reflect_ref as RR
from sdf3d_amd import abi, scenes
from sdf3d_amd.camera import Arcball

EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
C4_GRID = ((-1.13, -0.11, -1.02), (0.12, 0.08, 0.11), (19, 11, 17))   # the mesh tests' grid on C4
CARVED = 6            # the primitive of C4 whose operator C4-carved changes
LIGHTS = LR.rig(8)
SHAPES = {2: (37, 23), 4: (21, 10)}    # output W x H of the S x S supersampled cases


def signature(scene):
    """The (kind, op) sequence the dispatcher matches against its variants."""
    return tuple((int(scene.prims[i].kind), int(scene.prims[i].op)) for i in range(scene.count))


# ---- random scenes ---------------------------------------------------------------------------

def custom_scene(rng, n, w=160, h=90):
    """n random primitives after the plane, random kinds and (union-family or
    CSG) ops: signatures no built-in variant has."""
    f = scenes.config("C3", w, h)
    f.scene.count = 1 + n
    kinds = [abi.PRIM_SPHERE, abi.PRIM_BOX, abi.PRIM_ROUND_BOX, abi.PRIM_TORUS,
             abi.PRIM_CAPSULE, abi.PRIM_CYLINDER]
    for i in range(1, 1 + n):
        p = f.scene.prims[i]
        p.kind = int(rng.choice(kinds))
        p.op = int(rng.choice([abi.OP_UNION, abi.OP_SMOOTH_UNION, abi.OP_SMOOTH_UNION,
                               abi.OP_SUBTRACT, abi.OP_INTERSECT, abi.OP_SMOOTH_SUBTRACT]))
        p.k = float(rng.uniform(0.02, 0.4))
        c = rng.uniform(-0.8, 0.8, 3) + np.array([0.0, 0.45, 0.0])
        vals = list(c) + list(rng.uniform(0.08, 0.3, 6))
        if p.kind == abi.PRIM_CAPSULE:
            vals = list(c) + list(c + rng.uniform(-0.4, 0.4, 3)) + [float(rng.uniform(0.05, 0.15))]
        if p.kind == abi.PRIM_ROUND_BOX:
            vals[6] = float(rng.uniform(0.01, 0.05))
        for j, v in enumerate(vals[:9]):
            p.p[j] = float(v)
    return f


def random_csg8(rng, spread, kmax):
    """A scene with the CSG8 signature (so the culled FixedScene variant runs)
    but random sizes, positions and blend radii."""
    f = scenes.config("C3", 160, 96)
    s = f.scene
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    c = lambda: (u(-spread, spread), u(-0.2, spread), u(-spread, spread))  # noqa: E731
    s.prims[0].p[3] = u(-0.3, 0.3)                                  # plane offset
    for i in range(1, 8):
        pr = s.prims[i]
        pr.k = u(1e-3, kmax)
        x, y, z = c()
        pr.p[0], pr.p[1], pr.p[2] = x, y, z
        kind = pr.kind
        if kind == abi.PRIM_SPHERE:
            pr.p[3] = u(0.01, 0.6)
        elif kind in (abi.PRIM_BOX, abi.PRIM_ROUND_BOX):
            pr.p[3], pr.p[4], pr.p[5] = u(0.02, 0.5), u(0.02, 0.5), u(0.02, 0.5)
            if kind == abi.PRIM_ROUND_BOX:
                pr.p[6] = u(0.0, 0.5) * min(pr.p[3], pr.p[4], pr.p[5])
        elif kind == abi.PRIM_TORUS:
            pr.p[3], pr.p[4] = u(0.05, 0.5), u(0.01, 0.2)
        elif kind == abi.PRIM_CAPSULE:
            pr.p[3], pr.p[4], pr.p[5] = c()
            pr.p[6] = u(0.01, 0.3)
        elif kind == abi.PRIM_CYLINDER:
            pr.p[3], pr.p[4] = u(0.02, 0.4), u(0.02, 0.6)
    return f


def random_scene(rng, n):
    """The plane and n - 1 random primitives under (mostly smooth) union, up to
    3 from the origin: the scenes of the bounds tests."""
    f = scenes.config("C3", 64, 64)
    s = f.scene
    C.memset(C.addressof(s.prims), 0, C.sizeof(s.prims))
    s.count = n
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    s.prims[0].kind, s.prims[0].op = abi.PRIM_PLANE, abi.OP_UNION
    s.prims[0].p[1] = 1.0
    kinds = [abi.PRIM_SPHERE, abi.PRIM_BOX, abi.PRIM_ROUND_BOX, abi.PRIM_TORUS,
             abi.PRIM_CAPSULE, abi.PRIM_CYLINDER]
    for i in range(1, n):
        pr = s.prims[i]
        pr.kind = kinds[int(rng.integers(len(kinds)))]
        pr.op = abi.OP_SMOOTH_UNION if rng.random() < 0.8 else abi.OP_UNION
        pr.k = u(1e-3, 0.5)
        for j in range(3):
            pr.p[j] = u(-3, 3)
        if pr.kind == abi.PRIM_CAPSULE:
            for j in range(3, 6):
                pr.p[j] = u(-3, 3)
            pr.p[6] = u(0.01, 0.5)
        else:
            for j in range(3, 6):
                pr.p[j] = u(0.01, 1.0)
            pr.p[6] = u(0.0, 0.05)
    return f.scene


# ---- the scripted navigation of the host program ------------------------------------------------

def nav_input(a: Arcball, i: int):
    """The scripted navigation input of frame i (examples/sdf_main.cpp nav_input)."""
    dt = 1.0 / 60.0
    ph = i % 90
    if ph < 30:
        return a.update(dt, 0.004, 0.0015, orbit=True)
    if ph < 45:
        return a.update(dt, -0.002, 0.001, pan=True)
    if ph < 60:
        return a.update(dt)
    if ph < 80:
        return a.gamepad(dt, 0.8, -0.5, 0.2, 0.35)
    return a.gamepad(dt, 0.1, 0.0, 0.0, 0.0)


def nav_views(n: int) -> np.ndarray:
    a = Arcball()
    return np.stack([nav_input(a, i) for i in range(n)])


# ---- run-time specialised scenes: three primitives on C3's pose 2 ----------------------------------

def _three(prec, wh, prims):
    """C3's frame, pose 2, with its scene replaced by `prims`: (kind, op, k, p...)."""
    f = scenes.config("C3", *wh, precision=prec, pose=2)
    C.memset(C.addressof(f.scene.prims), 0, C.sizeof(f.scene.prims))
    f.scene.count = len(prims)
    for i, (kind, op, *rest) in enumerate(prims):
        scenes._prim(f.scene, i, kind, op, *rest)
    return f


PLANE = (abi.PRIM_PLANE, abi.OP_UNION, 0.0, 0.0, 1.0, 0.0, 0.0)


def unmatched_scene(s, prec):
    """C3's plane, box, torus in hard union at the supersampled shape of S (the
    ssaa tests; one kernel serves both S, which is a uniform)."""
    f = scenes.config("C3", *SHAPES[s], precision=prec, pose=2)
    f.params.samples = s
    f.scene.count = 3
    scenes._prim(f.scene, 1, abi.PRIM_BOX, abi.OP_UNION, 0.0, -0.4, 0.15, 0.0, 0.15, 0.15, 0.15)
    scenes._prim(f.scene, 2, abi.PRIM_TORUS, abi.OP_UNION, 0.0, 0.4, 0.1, 0.0, 0.2, 0.06)
    return f


def specialised_scene(prec):
    """C3's plane, torus, box in hard union (the lights tests): unmatched_scene
    with the primitives in another order."""
    f = scenes.config("C3", *LR.SHAPE, precision=prec, pose=2)
    f.scene.count = 3
    scenes._prim(f.scene, 1, abi.PRIM_TORUS, abi.OP_UNION, 0.0, 0.4, 0.1, 0.0, 0.2, 0.06)
    scenes._prim(f.scene, 2, abi.PRIM_BOX, abi.OP_UNION, 0.0, -0.4, 0.15, 0.0, 0.15, 0.15, 0.15)
    return f


def hard_union(prec, wh=MR.SHAPE, swapped=False):
    """plane, capsule, box in hard union (`swapped`: plane, box, capsule); the
    materials tests, which count `swapped`."""
    cap = (abi.PRIM_CAPSULE, abi.OP_UNION, 0.0, -0.4, 0.1, 0.2, 0.3, 0.4, -0.1, 0.12)
    box = (abi.PRIM_BOX, abi.OP_UNION, 0.0, 0.5, 0.15, 0.1, 0.15, 0.15, 0.15)
    return _three(prec, wh, [PLANE, box, cap] if swapped else [PLANE, cap, box])


def mirror_scene(prec, wh=RR.SHAPE, swapped=False):
    """plane, round box (hard union), torus (smooth union) -- `swapped`: plane,
    torus, round box; the reflect tests, which count `swapped`."""
    box = (abi.PRIM_ROUND_BOX, abi.OP_UNION, 0.0, -0.4, 0.25, 0.1, 0.2, 0.2, 0.2, 0.05)
    tor = (abi.PRIM_TORUS, abi.OP_SMOOTH_UNION, 0.08, 0.45, 0.12, 0.0, 0.25, 0.08)
    return _three(prec, wh, [PLANE, tor, box] if swapped else [PLANE, box, tor])


def _around_the_plane(prec, wh, a, b):
    """a (hard union), plane, b (smooth union 0.08); a, b: (kind, p...)."""
    return _three(prec, wh, [(a[0], abi.OP_UNION, 0.0, *a[1:]), PLANE,
                             (b[0], abi.OP_SMOOTH_UNION, 0.08, *b[1:])])


TORUS = (abi.PRIM_TORUS, 0.45, 0.12, 0.0, 0.25, 0.08)


def env_scene(prec, wh=ER.SHAPE, counted=False):
    """round box, plane, torus (smooth union) -- `counted`: torus, plane, round
    box (smooth union); the env and rays tests, of which env counts `counted`."""
    box = (abi.PRIM_ROUND_BOX, -0.4, 0.25, 0.1, 0.2, 0.2, 0.2, 0.05)
    return _around_the_plane(prec, wh, *((TORUS, box) if counted else (box, TORUS)))


def points_scene(prec, counted=False):
    """capsule, plane, torus (smooth union) -- `counted`: torus, plane, capsule;
    the points tests, which count `counted`."""
    cap = (abi.PRIM_CAPSULE, -0.4, 0.15, 0.1, 0.1, 0.5, -0.1, 0.12)
    f = _around_the_plane(prec, MR.SHAPE, *((TORUS, cap) if counted else (cap, TORUS)))
    f.params.dispatch = abi.DISPATCH_AUTO
    return f


def rays_scene(prec=EXACT):
    """cylinder, plane, capsule (smooth union); the rays tests count it."""
    f = _around_the_plane(prec, ER.SHAPE, (abi.PRIM_CYLINDER, -0.4, 0.25, 0.1, 0.18, 0.25),
                          (abi.PRIM_CAPSULE, 0.3, 0.1, 0.1, 0.7, 0.35, 0.0, 0.08))
    f.params.dispatch = abi.DISPATCH_AUTO
    return f


def rays_jit_case():
    """(frame, shading) of the rays test that counts rays_scene's compilations,
    in the test's process and in the child it starts."""
    f = rays_scene()
    return f, dict(lights=LIGHTS[:2], light_flags=abi.LIGHTS_COLOR, materials=mats_of(f),
                   reflect=RR.reflect(2, 0.75),
                   env=ER.environment(abi.ENV_SKY | abi.ENV_SUN | abi.ENV_FOG))


# ---- frames by name --------------------------------------------------------------------------------

def frame_of(name, pose, prec=EXACT, dispatch=None):
    """The frame `name` of the materials and reflect tests (materials_ref.FRAMES,
    C5, HU: hard_union, or RJ: mirror_scene).  SIX and SIXH run the generic
    kernel unless `dispatch` says otherwise."""
    if name in ("HU", "RJ"):
        f = hard_union(prec) if name == "HU" else mirror_scene(prec)
    elif name == "C5":
        f = scenes.config("C5", *RR.SHAPE, precision=prec, pose=pose)
    else:
        f = MR.frame_of(name, pose, prec)
    if dispatch is None:
        dispatch = abi.DISPATCH_GENERIC if name in ("SIX", "SIXH") else abi.DISPATCH_AUTO
    f.params.dispatch = dispatch
    return f


def the_frame(name, pose, prec=EXACT, dispatch=None):
    """frame_of, and EJ: env_scene (the env and rays tests)."""
    if name == "EJ":
        f = env_scene(prec)
        f.params.dispatch = abi.DISPATCH_AUTO if dispatch is None else dispatch
        return f
    return frame_of(name, pose, prec, dispatch)


def mats_of(f):
    return MR.palette_for(f) if f.scene.kind == abi.SCENE_PRIMITIVES else [f.material]


def fast_case(name, dispatch=None):
    """(frame in fast precision, materials) of the env and rays tests' fast
    cases.  `dispatch` None: the frame's own launch path (a built-in variant,
    EJ's run-time specialised kernel, the Mandelbulb's unit).  REF and C5 take
    the one-material form."""
    f = the_frame(name, {"C4": 0, "C3": 2, "REF": 0, "EJ": 2, "C5": 0}[name], FAST, dispatch)
    mats = (RR.materials_for(f) if name in ("REF", "C5") else MR.palette_for(f))
    return f, mats


_WALK = {}


def walk_of(name, pose, bounces, n, flags):
    """The CPU reference's walk of the_frame(name, pose) under the first n
    LIGHTS, strength 1, with its layer colours: computed once, read-only."""
    key = (name, pose, bounces, n, flags)
    if key not in _WALK:
        f = the_frame(name, pose)
        w = RR.walk(f, mats_of(f), bounces, 1.0, LIGHTS[:n])
        w["C"] = RR.layer_colours(f, w, flags)
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WALK[key] = w
    return _WALK[key]


def c4_path(dispatch, carved=False):
    """A factory (prec, wh) of C4 on a launch path; `carved`: with primitive
    CARVED carved out of the rest instead of blended into it (fast_paths.py)."""
    def make(prec=EXACT, wh=(64, 36)):
        f = scenes.config("C4", *wh)
        if carved:
            f.scene.prims[CARVED].op = abi.OP_SMOOTH_SUBTRACT
        f.params.dispatch = dispatch
        f.params.precision = prec
        return f
    return make


# J<seed>: custom_scene(100 + seed), signatures with CSG operators that no
# built-in variant has (run-time specialised under SDF_DISPATCH_AUTO)
JIT_SEEDS = {"J0": 0, "J4": 4, "J6": 6}


def query_frame(kind, prec=EXACT, wh=(64, 36)):
    """The frames of the query, mesh and offset tests: a built-in scene, with
    -generic or -unculled on that dispatch path, J<seed>, or C4-carved."""
    if kind in JIT_SEEDS:
        seed = JIT_SEEDS[kind]
        f = custom_scene(np.random.default_rng(100 + seed), 2 + seed % 7, *wh)
    elif kind == "C4-carved":       # run-time specialised, with C4's arithmetic (fast_paths.py)
        f = c4_path(abi.DISPATCH_AUTO, carved=True)(prec, wh)
    else:
        f = scenes.config(kind.split("-")[0], *wh)
        if kind.endswith("-generic"):
            f.params.dispatch = abi.DISPATCH_GENERIC
        if kind.endswith("-unculled"):
            f.params.dispatch = abi.DISPATCH_UNCULLED
    f.params.precision = prec
    return f


# ---- the scenes whose compilations are counted -------------------------------------------------------

# test (file: name) -> the scene it counts
COUNTED = {
    "ssaa: test_runtime_specialised_scene": lambda: unmatched_scene(2, EXACT),
    "lights: test_runtime_specialised_scene": lambda: specialised_scene(EXACT),
    "materials: test_runtime_specialised_scene_compiles_one_kernel":
        lambda: hard_union(EXACT, swapped=True),
    "reflect: test_runtime_specialised_scene_compiles_one_kernel":
        lambda: mirror_scene(EXACT, swapped=True),
    "env: test_runtime_specialised_scene_compiles_one_kernel":
        lambda: env_scene(EXACT, counted=True),
    "points: test_the_run_time_compiled_kernel_is_counted":
        lambda: points_scene(EXACT, counted=True),
    "rays: test_runtime_specialised_scene_compiles_one_kernel": rays_scene,
    # rays' fast case EJ counts env_scene's rays kernel (fast_paths.first_use)
    "rays: test_fast_is_near_the_reference[EJ]": lambda: env_scene(FAST),
    **{f"query, mesh: {k}": (lambda k=k: query_frame(k)) for k in JIT_SEEDS},
}
# run-time specialised too, rendered by several tests, counted by none
UNCOUNTED = {
    "materials: HU": lambda: hard_union(EXACT),
    "reflect: RJ": lambda: mirror_scene(EXACT),
    "points: PJ": lambda: points_scene(EXACT),
}
