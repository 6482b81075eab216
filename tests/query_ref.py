"""Reference of the query entry points (include/sdf_abi.h "Queries":
sdf_trace, sdf_trace_camera, sdf_sample), in NumPy over the CPU oracle's point
probes (oracle.raymarch, oracle.normal, oracle.scene_sdf, oracle.uniforms).
TEST INFRASTRUCTURE ONLY.

Every value is fp32, every operation rounded once, nothing fused: NumPy's
float32 element-wise arithmetic and its correctly rounded sqrt are the exact
precision's operations.

  normalize    sqrt((x x + y y) + z z), then three divisions
  march        oracle.raymarch per ray
  replay       the march forced to k iterations, break tests ignored:
               d = f32(d + scene_sdf(f32(O + f32(D d))))
  owner        the owner fold from truncated scenes: the running d before
               primitive i is scene_sdf of the scene cut to its first i
               primitives (+INF for i = 0), v_i is scene_sdf of the
               one-primitive scene {primitive i, UNION}
  camera_rays  the pixel rays restated from oracle.uniforms and the oracle's
               row loop (oracle_core.h render_rows)
"""
import ctypes as C

import numpy as np

import oracle
from sdf3d_amd import abi

f32 = np.float32
INF = f32(np.inf)
SEED, N_RAYS = 7, 200


def normalize(v):
    """fp32 normalize of (n, 3): the left-to-right sum of three rounded
    products, an IEEE square root, three IEEE divisions."""
    v = np.ascontiguousarray(v, dtype=f32)
    with np.errstate(all="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        l = np.sqrt((x * x + y * y) + z * z)
        return np.stack([x / l, y / l, z / l], axis=1).astype(f32)


def ray_set(seed=SEED, n=N_RAYS):
    """The random ray set of the query tests: origins uniform in [-2.5, 2.5]^2
    with y in [0.05, 2.5]; directions aimed at a point of [-1, 1]^2 x [-0.2, 1]
    and scaled by a factor in [0.1, 10]; every fifth direction Gaussian."""
    rng = np.random.default_rng(seed)
    o = np.empty((n, 3))
    o[:, 0] = rng.uniform(-2.5, 2.5, n)
    o[:, 1] = rng.uniform(0.05, 2.5, n)
    o[:, 2] = rng.uniform(-2.5, 2.5, n)
    tgt = np.empty((n, 3))
    tgt[:, 0] = rng.uniform(-1.0, 1.0, n)
    tgt[:, 1] = rng.uniform(-0.2, 1.0, n)
    tgt[:, 2] = rng.uniform(-1.0, 1.0, n)
    d = (tgt - o) * rng.uniform(0.1, 10.0, n)[:, None]
    g = rng.normal(size=(n, 3))
    d[::5] = g[::5]
    return np.ascontiguousarray(o, dtype=f32), np.ascontiguousarray(d, dtype=f32)


def hand_rays():
    """Five hand-made rays: a zero direction; an origin inside a primitive (the
    reference sphere, which every primitive scene here keeps); directions
    scaled by 1e-3 and 1e3; a ray grazing the floor."""
    o = np.array([[0.0, 0.5, 2.0], [0.0, 0.4, 0.0], [0.3, 0.6, 2.0], [-0.4, 0.7, 1.5],
                  [-2.0, 0.011, 0.1]], dtype=f32)
    d = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, 1.0], [-0.3e-3, -0.4e-3, -2.0e-3],
                  [0.3e3, -0.5e3, -1.5e3], [1.0, -0.002, 0.0]], dtype=f32)
    return o, d


ZERO_DIR = 0   # index of the zero direction among hand_rays()


def odd_rays():
    """Directions without a finite length: normalize gives them NaN components
    (INF / INF), some with finite (zero) ones beside, so the point marched has
    NaN and finite coordinates mixed."""
    inf, nan = np.inf, np.nan
    d = np.array([[inf, 0.0, 0.0], [0.0, -inf, 0.0], [nan, 1.0, 0.0], [1.0, 1.0, inf],
                  [0.0, 0.0, -inf], [-inf, inf, 0.0], [nan, nan, nan], [0.0, 0.0, 0.0]], dtype=f32)
    o = np.tile(np.array([[0.3, 0.6, 2.0]], dtype=f32), (len(d), 1))
    o[1] = [0.0, 0.4, 0.05]       # inside the reference sphere
    o[4] = [-0.7, 0.15, 0.5]
    return o, d


def march(frame, O, D):
    """(t float32 (n,), steps int32 (n,)) of oracle.raymarch along unit D."""
    n = len(O)
    t = np.empty(n, dtype=f32)
    st = np.empty(n, dtype=np.int32)
    for i in range(n):
        t[i], st[i] = oracle.raymarch(frame.scene, frame.params, O[i], D[i])
    return t, st


def _sdf(scene, P):
    return np.array([oracle.scene_sdf(scene, float(p[0]), float(p[1]), float(p[2])) for p in P],
                    dtype=f32)


def scene_sdf(frame, P):
    return _sdf(frame.scene, np.asarray(P, dtype=f32))


def point(O, D, d):
    """P = O + D d as the march forms it."""
    with np.errstate(all="ignore"):
        d = np.asarray(d, dtype=f32)[:, None]
        return O.astype(f32) + D.astype(f32) * d     # float32 arrays: each operation rounds once


def replay(frame, O, D, k):
    """The march's distance after exactly k[i] iterations (k <= max_steps),
    whatever the break tests say."""
    O, D = np.asarray(O, dtype=f32), np.asarray(D, dtype=f32)
    k = np.minimum(np.asarray(k, dtype=np.int64), frame.params.max_steps)
    d = np.zeros(len(O), dtype=f32)
    with np.errstate(all="ignore"):
        for step in range(int(k.max()) if len(k) else 0):
            on = np.nonzero(step < k)[0]
            p = point(O[on], D[on], d[on])
            d[on] = (d[on] + _sdf(frame.scene, p)).astype(f32)
    return d


def normals(frame, P):
    return np.stack([oracle.normal(frame.scene, frame.params, p) for p in P]).astype(f32) \
        if len(P) else np.zeros((0, 3), dtype=f32)


def _cut(scene, n):
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(scene), C.sizeof(s))
    s.count = n
    return s


def _single(scene, i):
    s = abi.sdf_scene()
    C.memmove(C.addressof(s), C.addressof(scene), C.sizeof(s))
    s.count = 1
    C.memmove(C.addressof(s.prims[0]), C.addressof(scene.prims[i]), C.sizeof(abi.sdf_primitive))
    s.prims[0].op = abi.OP_UNION
    return s


def owner(frame, P):
    """(w int32 (n,), min_gap float64 (n,)): the owner fold at each point and
    the smallest |a - b| among its finite pairs (how close its closest
    decision was).  A Mandelbulb: 0 and +inf."""
    P = np.asarray(P, dtype=f32)
    n = len(P)
    w = np.zeros(n, dtype=np.int32)
    gap = np.full(n, np.inf)
    sc = frame.scene
    if sc.kind != abi.SCENE_PRIMITIVES:
        return w, gap
    with np.errstate(all="ignore"):
        for i in range(sc.count):
            d = np.full(n, INF, dtype=f32) if i == 0 else _sdf(_cut(sc, i), P)
            v = _sdf(_single(sc, i), P)
            op = sc.prims[i].op
            a = d if op in (abi.OP_UNION, abi.OP_SMOOTH_UNION) else -d
            b = -v if op in (abi.OP_INTERSECT, abi.OP_SMOOTH_INTERSECT) else v
            w[b < a] = i
            g = np.abs(a.astype(np.float64) - b.astype(np.float64))
            fin = np.isfinite(g)
            gap[fin] = np.minimum(gap[fin], g[fin])
    return w, gap


def hits(frame, O, D):
    """The reference of a traced ray set along unit directions D: dict of t,
    steps, normal, prim, the hit mask, P and min_gap."""
    O, D = np.asarray(O, dtype=f32), np.asarray(D, dtype=f32)
    t, st = march(frame, O, D)
    hit = ~(t > f32(frame.params.max_dist))     # a NaN distance is not a miss
    P = point(O, D, t)
    nrm = np.zeros((len(O), 3), dtype=f32)
    prim = np.full(len(O), -1, dtype=np.int32)
    gap = np.full(len(O), np.inf)
    idx = np.nonzero(hit)[0]
    nrm[idx] = normals(frame, P[idx])
    prim[idx], gap[idx] = owner(frame, P[idx])
    return {"t": t, "steps": st, "normal": nrm, "prim": prim, "hit": hit, "P": P, "min_gap": gap}


def trace(frame, origins, dirs):
    """sdf_trace's reference: D = normalize(dirs)."""
    return hits(frame, origins, normalize(dirs))


def fast_deviation(frame, origins, dirs, got, gap):
    """A fast-precision sdf_trace (`got`: t, steps, normal, prim as NumPy)
    against the reference, arithmetic only: `t` against the replay at the
    kernel's own step counts, on every ray, as |t - r| / max(1, |r|) (equal
    non-finite values deviate by 0, unequal ones by inf); `normal` as the
    largest absolute component difference on the hit rays whose steps agree
    with the oracle's; `prim` as the number of disagreements among the
    reference's hit rays whose closest owner decision is at least `gap` wide."""
    D = normalize(dirs)
    ref = hits(frame, origins, D)
    rep = replay(frame, origins, D, got["steps"])
    t = np.asarray(got["t"], dtype=f32)
    with np.errstate(all="ignore"):
        same = (bits_of(t) == bits_of(rep)) | (np.isnan(t) & np.isnan(rep))
        dt = np.abs(t.astype(np.float64) - rep) / np.maximum(1.0, np.abs(rep.astype(np.float64)))
    dt = np.where(same, 0.0, np.where(np.isfinite(dt), dt, np.inf))
    agree = ref["hit"] & (got["steps"] == ref["steps"]) & ~(t > f32(frame.params.max_dist))
    with np.errstate(all="ignore"):
        dn = np.abs(got["normal"][agree].astype(np.float64) - ref["normal"][agree])
    dn = np.where(np.isnan(got["normal"][agree]) & np.isnan(ref["normal"][agree]), 0.0, dn)
    wide = ref["hit"] & (ref["min_gap"] >= gap)
    return {"t": float(dt.max()), "normal": float(dn.max()) if dn.size else 0.0,
            "normal_rays": int(agree.sum()), "hit": int(ref["hit"].sum()),
            "steps_differ": int((got["steps"] != ref["steps"]).sum()),
            "prim_wrong": int((got["prim"][wide] != ref["prim"][wide]).sum()),
            "prim_left_out": int((ref["hit"] & ~wide).sum())}


def bits_of(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def camera_rays(frame):
    """(O, D) of every pixel, entry y * W + x, as sdf_render forms them."""
    p = frame.params
    u = oracle.uniforms(frame.camera, p)
    W, H = p.width, p.height
    x = np.arange(W, dtype=np.int64)
    y = np.arange(H, dtype=np.int64)
    qx = (2 * x + 1).astype(f32) / f32(W) - f32(1)
    qy = (2 * y + 1).astype(f32) / f32(H) - f32(1)
    QX, QY = np.meshgrid(qx, qy)               # [y, x]
    v = np.stack([(QX * f32(u["aspect"])).ravel(), QY.ravel(),
                  np.full(W * H, f32(u["focal"]), dtype=f32)], axis=1).astype(f32)
    r0 = normalize(v)
    m = u["inv_view"].astype(f32)
    zero = f32(0)
    r1 = np.stack([((m[c] * r0[:, 0] + m[4 + c] * r0[:, 1]) + m[8 + c] * r0[:, 2]) + m[12 + c] * zero
                   for c in range(3)], axis=1).astype(f32)
    D = normalize(r1)
    O = np.tile(u["cam"].astype(f32), (W * H, 1))
    return O, D


def grid(lo=(-1.5, -0.3, -1.5), hi=(1.5, 1.2, 1.5), shape=(17, 13, 11)):
    """The 17 x 13 x 11 sample grid spanning the scenes: points inside
    primitives and below the floor included."""
    ax = [np.linspace(lo[i], hi[i], shape[i]) for i in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g, dtype=f32)
