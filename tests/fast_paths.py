"""What the fast-precision tests of the launch paths share (DESIGN.md "Which
test holds which launch path"): the frames of the paths, and the comparison of
a fast sdf_sample with the oracle.  TEST INFRASTRUCTURE ONLY.

A fast case on a path is held by three things: a bound the project already
asserts for the same arithmetic, with the oracle as reference, on a scene built
from the primitives and operators of the scene that bound was measured on; the
fast output differing in at least one bit from the exact output of the same
call, which is itself held to the oracle bit for bit (so equal bits mean the
exact kernel ran); and, on a run-time specialised scene, the count of
compilations.  No bound is derived from the kernels under test.

C4-carved is C4 with primitive 6, the round box, carved out of the rest
(SDF_OP_SMOOTH_SUBTRACT) instead of blended into it: the kinds and the smooth
kernel of C4, a signature no built-in variant has, and distances the built-in
C4 kernel does not give (340 of the 2431 grid points differ by more than
7.7e-5, t on the 200-ray set by up to 0.35: tests/test_fast_paths_ref.py).
Swapping two primitives of a smooth-union chain, the run-time specialised scene
of test_gpu_frames.py, changes owners but hardly a distance."""
import os

import numpy as np

import oracle
import query_ref as Q
from cases import CARVED, the_frame  # noqa: F401 (CARVED: for the tests)
from cases import c4_path as _c4
from sdf3d_amd import abi

f32 = np.float32
LEFT_OUT_SHARE = 0.02

# ---- the fast bounds that more than one module reads (query, mesh, env) ---------------------------

# Fast precision against the reference (query_ref.fast_deviation) on the
# 200-ray set over REF, C4 and C5, measured on an MI355X
# (profiles/query_C4.json fast_deviation, DESIGN.md "query"): the largest
# deviation of `t` from the replay at the kernel's own step counts, relative to
# max(1, |t|), and the largest absolute difference of a normal's component on
# the rays whose steps agree with the oracle's.  The bounds asserted are 4 x
# those, the headroom test_gpu_env.py, test_gpu_reflect.py and
# test_gpu_materials.py give theirs (compiler versions contract differently;
# the inputs are fixed).
# (REF 4.72e-7 / 1.25e-6, C4 5.03e-6 / 5.96e-6, C5 1.919e-5 / 6.752e-5; no ray's
# step count differed from the oracle's, no owner was wrong, none was left out)
FAST_MEASURED_T = 1.919e-5
FAST_MEASURED_N = 6.752e-5
FAST_BOUND_T = 4 * FAST_MEASURED_T
FAST_BOUND_N = 4 * FAST_MEASURED_N
# Fast precision against the reference on the two grids whose lattice keeps
# min |w| >= 1e-4 (no sign can flip), measured on an MI355X
# (profiles/mesh_C4.json fast_deviation): the largest |vertex - reference| /
# cell over the components, and the largest normal-component difference.  The
# bounds asserted are 4 x those, the headroom test_gpu_query.py gives its own.
# (C1 1.788e-6 / 1.341e-6, C4 1.614e-6 / 4.195e-6; no owner differed)
MESH_MEASURED_V = 1.789e-6
MESH_MEASURED_N = 4.195e-6
MESH_BOUND_V = 4 * MESH_MEASURED_V
MESH_BOUND_N = 4 * MESH_MEASURED_N
# Fast precision's composite against the reference replayed at the kernel's
# per-layer step counts, on the pixels away from the miss boundary
# (env_ref.near_boundary): the largest absolute deviation of a channel measured
# on an MI355X over C4 pose 0, C3 pose 2 (palette) and REF pose 0 (one
# material), bounces 1 and 2, SKY | SUN | FOG (profiles/env_C4.json
# fast_deviation, DESIGN.md "Environment"), and the bound asserted: 4 x that,
# the headroom test_gpu_reflect.py and test_gpu_materials.py give theirs.
ENV_MEASURED = 1.253e-4
ENV_BOUND = 4 * ENV_MEASURED
WEIGHT = abi.REFLECT_WEIGHT
ALL = abi.ENV_SKY | abi.ENV_SUN | abi.ENV_FOG


def _env(name, pose, dispatch=None):
    def make(prec=abi.PRECISION_EXACT, wh=None):
        return the_frame(name, pose, prec, dispatch)      # its shape is env_ref.SHAPE
    return make


# name -> frame factory (prec, wh).  The first three are cases.query_frame's
# kinds; the rays-* ones are cases.the_frame's (EJ: round box, plane, torus
# under smooth union, run-time specialised; kinds C4 has).
PATHS = {
    "C4-generic": _c4(abi.DISPATCH_GENERIC),
    "C4-unculled": _c4(abi.DISPATCH_UNCULLED),
    "C4-carved": _c4(abi.DISPATCH_AUTO, carved=True),
    "rays-C4-generic": _env("C4", 0, abi.DISPATCH_GENERIC),
    "rays-C4-unculled": _env("C4", 0, abi.DISPATCH_UNCULLED),
    "rays-EJ": _env("EJ", 2),
    "rays-C5": _env("C5", 0),
}
JIT = ("C4-carved", "rays-EJ")      # run-time specialised under SDF_DISPATCH_AUTO


def jit_on():
    return os.environ.get("SDF3D_JIT") != "0"


_compiled = set()


def first_use(key):
    """How many run-time compilations the first call of `key` (a family's kernel
    on a JIT path in fast precision, as the caller names it) must make: 1 the
    first time the key is asked about in this process, then 0."""
    n = 1 if jit_on() and key not in _compiled else 0
    _compiled.add(key)
    return n


# ---- sdf_sample against the oracle ------------------------------------------------

_REF = {}


def point_reference(frame, P):
    """dist and normal of the fp32 oracle at P, and the normals of its two
    other readings (contracted fp32, the fp64 twin), computed once per scene
    and point set and shared read-only."""
    p = frame.params
    key = (bytes(frame.scene), p.normal_mode, p.normal_eps, P.tobytes())
    if key not in _REF:
        r = {"dist": Q.scene_sdf(frame, P), "normal": Q.normals(frame, P)}
        for reading in ("fma", "f64"):
            r[reading] = np.stack([oracle.normal(frame.scene, p, q, reading=reading) for q in P])
        for a in r.values():
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _absdiff(a, b):
    """|a - b| in fp64; NaN against NaN is 0, NaN against a number inf."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


def point_deviation(frame, P, dist, normal):
    """An sdf_sample result (dist (n,), normal (n, 3) as NumPy) at the points P
    against the oracle: `dist` the largest |dist - ref| / max(1, |ref|) over all
    points (equal non-finite values deviate by 0, unequal ones by inf, as
    query_ref.fast_deviation treats t); `normal` the largest absolute component
    difference over the points kept; `normal_left_out` the points not kept.  A
    point is kept unless the normal of one of the oracle's other readings (the
    contracted fp32 one, the fp64 twin) differs from the fp32 oracle's by more
    than FAST_BOUND_N / 4 in some component: there the normal
    depends on the rounding the reference leaves open (a gradient near zero)."""
    P = np.ascontiguousarray(P, dtype=f32)
    ref = point_reference(frame, P)
    dist, r = np.asarray(dist, dtype=f32), ref["dist"]
    with np.errstate(all="ignore"):
        same = (Q.bits_of(dist) == Q.bits_of(r)) | (np.isnan(dist) & np.isnan(r))
        dd = np.abs(dist.astype(np.float64) - r) / np.maximum(1.0, np.abs(r.astype(np.float64)))
    dd = np.where(same, 0.0, np.where(np.isfinite(dd), dd, np.inf))
    keep = np.ones(len(P), dtype=bool)
    for reading in ("fma", "f64"):
        keep &= (_absdiff(ref[reading], ref["normal"]) <= FAST_BOUND_N / 4).all(axis=1)
    dn = _absdiff(np.asarray(normal, dtype=f32)[keep], ref["normal"][keep])
    return {"dist": float(dd.max()) if dd.size else 0.0,
            "normal": float(dn.max()) if dn.size else 0.0,
            "normal_left_out": int((~keep).sum()), "points": len(P)}
