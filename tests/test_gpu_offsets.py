"""GPU tests of exact-precision culling on unit-size scenes far from the origin
(tests/offsets.py: whole frames moved by T, not scaled, to coordinates of 1e3,
1e4, 1e5 and 2^20 along three directions, and T = 0 as the control).

Everything here is exact precision and bit for bit, step counts included
where the call returns them: against the CPU oracle, which takes the same
translated frame and so stays the definition of the result, and against the
unculled dispatch of the same frame.

  render       C4 on the fixed kernel (cached gaps; shadow, AO; two poses; with
               and without step counts, the latter taking the shadow march's
               lit tail), two random scenes of the CSG8 signature, C4 on the
               generic kernel, the run-time specialised C4-carved, and one
               frame each through sdf_render_materials and sdf_render_reflect
  sdf_sample   at the adversarial points of tests/test_offsets.py -- chosen, not
               hoped for: beyond each cullable primitive's farthest feature,
               with a competitor whose value sweeps across the primitive's -- on
               the generic kernel culled and unculled and, for a capsule, a box
               and a sphere of CSG8-signature scenes, on the fixed kernel
  sdf_trace    the translated camera's rays, 256 rays from inside the cluster
               sphere and 256 grazing it
  sdf_render_rays, sdf_mesh_count / sdf_mesh_emit (brick skipping and dense)

96 x 54 frames, a 24^3 grid, a few thousand points per case.  A guard holds
that the frames still show something: by the oracle alone, at least 20 % of
each frame's pixels end on a cullable primitive."""
import numpy as np
import pytest

import env_ref as ER
import materials_ref as MR
import mesh_ref as M
import offsets as O
import oracle
import query_ref as Q
import reflect_ref as RR
from gpu_support import bitwise_eq, raw_mesh, sample, trace
from gpu_support import mesh_mismatches as mismatches
from sdf3d_amd import abi, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = list(O.OFFSETS)
MIN_SHARE = 0.20
MIN_FAR = 100


def unculled(f):
    g = f.copy()
    g.params.dispatch = abi.DISPATCH_UNCULLED
    return g


def unequal(a, b):
    """The number of entries that differ, NaN equal to NaN."""
    return int((~bitwise_eq(np.asarray(a), np.asarray(b))).sum())


# ---- render -------------------------------------------------------------------------
def extras(case, f):
    if case == "materials":
        return {"materials": MR.palette_for(f)}
    if case == "reflect":
        return {"materials": MR.palette_for(f), "reflect": RR.reflect(1, 1.0)}
    return {}


def gpu_render(rd, f, case, steps=True):
    out, st = rd.render(f, steps=steps, **extras(case, f))
    rd.torch.cuda.synchronize()
    return out.cpu().numpy(), (st.cpu().numpy() if steps else None)


def reference(case, f):
    if case in ("materials", "reflect"):
        rgba, steps, _ = RR.render(f, MR.palette_for(f), 1 if case == "reflect" else 0, 1.0)
        return rgba, steps
    return oracle.render(f)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", O.RENDER_CASES)
def test_render_equals_the_oracle_and_unculled(renderer, case, name):
    """The frame and its step counts equal the oracle's and the unculled
    dispatch's on every pixel; the render without a steps buffer (the bench's
    instantiation, whose shadow march ends at its lit tail) gives the same
    colours.

    reflect at 2^20 also holds the reflected layers' march of a NaN ray: the
    coordinates there are 0.125 apart, the normal's taps P +- h (h =
    normal_eps) all round to P, the normal is normalize(0) = NaN and so are
    the mirrored ray and its origin.  The reference marches such a ray for all
    max_steps (C4's smooth unions keep the NaN); a reflected layer that
    marched it through the scene evaluators' hardware minima stopped after one
    step, on 662, 3683 and 122 of the 5184 pixels of the three 2^20 frames
    (render_kernel.inc trace_march_path is the fix)."""
    f = O.case_frame(case, name)
    got, st = gpu_render(renderer, f, case)
    fast_path, _ = gpu_render(renderer, f, case, steps=False)
    plain, pst = gpu_render(renderer, unculled(f), case)
    ref, rst = reference(case, f)
    bad = {"oracle": unequal(got, ref), "oracle_steps": unequal(st, rst),
           "unculled": unequal(got, plain), "unculled_steps": unequal(st, pst),
           "no_steps": unequal(fast_path, got)}
    print(f"{case} at {name}: {got.shape[0] * got.shape[1]} pixels; words differing {bad}")
    if bad["oracle_steps"]:
        off = (st != rst)
        nan = np.isnan(ref[..., :3]).any(axis=-1)
        print(f"  step counts differ on {int(off.any(axis=-1).sum())} pixels (primary "
              f"{int(off[..., 0].sum())}, shadow {int(off[..., 1].sum())}), "
              f"{int((off.any(axis=-1) & nan).sum())} of them NaN in the reference's colour; "
              f"largest difference {int(np.abs(st - rst).max())}")
    assert bad == {"oracle": 0, "oracle_steps": 0, "unculled": 0, "unculled_steps": 0,
                   "no_steps": 0}


# ---- a reflected layer whose ray is NaN, through every kernel that marches one ------------
_nan_ref = {}


def nan_ray_reference(name, eflags):
    """(frame, materials, env, reference rgba, steps, pixels whose layer 1 the
    reference reaches with a NaN ray) of C4 at `name`, 1 bounce."""
    key = (name, eflags)
    if key not in _nan_ref:
        f = O.case_frame("reflect", name)
        mats = MR.palette_for(f)
        env = ER.environment(eflags) if eflags else None
        rgba, steps, e = ER.render(f, mats, 1, 1.0, env)
        w = e["walk"]
        nan = e["alive"][:, :, 1] & np.isnan(w["D"][:, :, 1]).all(axis=-1)
        _nan_ref[key] = (f, mats, env, rgba, steps, nan)
    return _nan_ref[key]


@pytest.mark.parametrize("name", ["2^20-xz", "2^20-skew"])
@pytest.mark.parametrize("eflags", [0, ER.SKY | ER.SUN, ER.SKY | ER.SUN | ER.FOG],
                         ids=["reflect", "sky", "sky-fog"])
@pytest.mark.parametrize("entry", ["frame", "rays"])
def test_nan_ray_layers_march_as_the_reference(renderer, entry, eflags, name):
    """At 2^20 the normal of many hit pixels is normalize(0) = NaN and layer 1's
    ray and origin are NaN.  Every kernel that marches such a layer gives the
    reference's colours and step counts (tests/env_ref.py over the walk of
    tests/reflect_ref.py): sdf_render_reflect and sdf_render_env (frame), and
    sdf_render_rays without and with an environment on the frame's own camera
    rays (rays), culled and unculled.  The case has a subject: by the
    reference alone, at least 100 pixels reach layer 1 with a NaN ray."""
    f, mats, env, ref, rst, nan = nan_ray_reference(name, eflags)
    assert int(nan.sum()) >= 100
    bad = {}
    for label, g in (("culled", f), ("unculled", unculled(f))):
        kw = dict(materials=mats, reflect=RR.reflect(1, 1.0), env=env)
        if entry == "frame":
            out, st = renderer.render(g, steps=True, **kw)
        else:
            o, d = renderer.camera_rays(g)
            out, st = renderer.render_rays(g, o.reshape(-1, 3), d.reshape(-1, 3), unit=True,
                                           steps=True, **kw)
        renderer.torch.cuda.synchronize()
        out, st = out.cpu().numpy().reshape(ref.shape), st.cpu().numpy().reshape(rst.shape)
        bad[label] = (unequal(out, ref), unequal(st, rst))
    print(f"{entry} eflags={eflags} at {name}: {int(nan.sum())} pixels with a NaN layer-1 ray; "
          f"words differing from the reference (colour, steps) {bad}")
    assert bad == {"culled": (0, 0), "unculled": (0, 0)}


@pytest.mark.parametrize("name", NAMES)
def test_frames_still_show_the_primitives(name):
    """By the oracle alone: at least 20 % of the pixels of every rendered case
    end on a cullable primitive (a march that ended below eps, owned by a
    primitive of the culled suffix)."""
    for case in O.RENDER_CASES:
        if case in ("C4-generic", "reflect"):       # C4-p0's scene and camera
            continue
        share = O.coverage(O.case_frame(case, name))
        print(f"{case} at {name}: {share:.3f} of the pixels on a cullable primitive")
        assert share >= MIN_SHARE, (case, name)


# ---- sdf_sample at the adversarial points --------------------------------------------
def probe(rd, scene, P, dispatch):
    f = scenes.config("C3", 64, 64)
    f.scene = scene
    f.params.dispatch = dispatch
    return sample(rd, f, P, normal=False)["dist"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind,op", O.CULLABLE,
                         ids=[f"{abi.PRIM_NAMES[k]}-{abi.OP_NAMES[o]}" for k, o in O.CULLABLE])
def test_generic_sample_at_shell_points(renderer, kind, op, name):
    """[competitor, primitive] scenes on the generic kernel, culled and
    unculled: the distance at every probe point equals the oracle's.  By the
    restated test alone, at least 100 of the points are far."""
    rng = np.random.default_rng(4321 + 16 * kind + op)
    tmpl = scenes.config("C3", 64, 64).scene
    far = points = 0
    bad = {"culled": 0, "unculled": 0}
    for _ in range(40):
        s, P = O.pair_scene(tmpl, O.OFFSETS[name], rng, kind, op)
        ref = O.sdf_at(s, P)
        bad["culled"] += unequal(probe(renderer, s, P, abi.DISPATCH_GENERIC), ref)
        bad["unculled"] += unequal(probe(renderer, s, P, abi.DISPATCH_UNCULLED), ref)
        far += int(O.says_far(s, 1, P)[0].sum())
        points += len(P)
        if far >= MIN_FAR:
            break
    print(f"{abi.PRIM_NAMES[kind]} {abi.OP_NAMES[op]} at {name}: {points} points, {far} far; "
          f"words differing from the oracle {bad}")
    assert bad == {"culled": 0, "unculled": 0}
    assert far >= MIN_FAR


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("which", list(O.CSG8_PROBED))
def test_fixed_kernel_sample_at_shell_points(renderer, which, name):
    """The same on the built-in fixed kernel: scenes of the CSG8 signature in
    which the probed primitive meets the head plane alone (offsets.csg8_probe).
    dist equals the oracle's and the unculled dispatch's.  The fixed kernel's
    plan is a gap-caching one, whose bounds carry kCullPath (|c|_inf + R + k +
    max_dist) beside the generic kernel's (0.01 at 1e4, 1.0 at 2^20): the
    probe's plane is lowered by up to 1.5 times that, and the at least 100 far
    points are counted by the restated test on a bracket of the plan's bounds
    (offsets.plan_bound), so they are far for the kernel that runs."""
    rng = np.random.default_rng(977 + O.CSG8_PROBED[which])
    tmpl = scenes.config("C4", 64, 64).scene
    reach = float(scenes.config("C3", 64, 64).params.max_dist)     # probe()'s frame
    far = far_generic = points = 0
    bad = {"fixed": 0, "unculled": 0}
    for _ in range(40):
        s, P, i = O.csg8_probe(tmpl, O.OFFSETS[name], rng, which, reach=reach)
        ref = O.sdf_at(s, P)
        bad["fixed"] += unequal(probe(renderer, s, P, abi.DISPATCH_AUTO), ref)
        bad["unculled"] += unequal(probe(renderer, s, P, abi.DISPATCH_UNCULLED), ref)
        far += int(O.says_far(s, i, P, reach=reach)[0].sum())
        far_generic += int(O.says_far(s, i, P)[0].sum())
        points += len(P)
        if far >= MIN_FAR and points - far >= MIN_FAR:
            break
    print(f"CSG8 {which} at {name}: {points} points, {far} far by the plan's bounds "
          f"({far_generic} by the generic kernel's); words differing from the oracle {bad}")
    assert bad == {"fixed": 0, "unculled": 0}
    assert far >= MIN_FAR and points - far >= MIN_FAR


# ---- sdf_trace ---------------------------------------------------------------------------
def cluster_rays(scene, rng, n=256):
    """n rays that start inside the scene's cluster sphere and n that graze it
    (closest approach within 2 % of its radius, from 1.5 to 4 radii away)."""
    rc, _, cl, _ = O.bounds_of(scene)
    assert rc == 0
    c, R = cl[:3].astype(np.float64), float(cl[3])

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    o_in = c + unit(n) * (R * rng.uniform(0, 0.95, n) ** (1 / 3))[:, None]
    d_in = unit(n)
    u = unit(n)
    w = np.cross(u, unit(n))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    touch = c + u * (R * rng.uniform(0.98, 1.02, n))[:, None]
    o_gr = touch - w * (R * rng.uniform(1.5, 4.0, n))[:, None]
    o = np.concatenate([o_in, o_gr]).astype(f32)
    d = np.concatenate([d_in, w * rng.uniform(0.5, 2.0, n)[:, None]]).astype(f32)
    return o, d


_trace_ref = {}


def trace_case(name, carved):
    """(frame, origins, dirs, reference) of the traced rays at offset `name`."""
    key = (name, carved)
    if key not in _trace_ref:
        f = O.case_frame("C4-carved" if carved else "C4-p0", name)
        co, cd = Q.camera_rays(f)
        ro, rdirs = cluster_rays(f.scene, np.random.default_rng(31))
        o, d = np.concatenate([co, ro]), np.concatenate([cd, rdirs])
        _trace_ref[key] = (f, o, d, Q.trace(f, o, d))
    return _trace_ref[key]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("path", ["C4", "C4-generic", "C4-carved"])
def test_trace_equals_the_oracle_and_unculled(renderer, path, name):
    """t, steps, normal and prim of caller-supplied rays whose origins lie far
    from the origin: the translated camera's own rays, 256 that start inside
    the cluster sphere and 256 that graze it."""
    f, o, d, ref = trace_case(name, path == "C4-carved")
    f = f.copy()
    if path == "C4-generic":
        f.params.dispatch = abi.DISPATCH_GENERIC
    got = trace(renderer, f, o, d)
    plain = trace(renderer, unculled(f), o, d)
    keys = ("t", "steps", "normal", "prim")
    bad = {k: unequal(got[k], ref[k]) for k in keys}
    bad_plain = {k: unequal(got[k], plain[k]) for k in keys}
    print(f"{path} at {name}: {len(o)} rays, {int(ref['hit'].sum())} hit; words differing from "
          f"the oracle {bad}, from unculled {bad_plain}")
    zero = dict.fromkeys(keys, 0)
    assert bad == zero and bad_plain == zero


# ---- sdf_render_rays ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_camera_rays_shade_to_the_translated_frame(renderer, name):
    """sdf_render_rays on the translated frame's sdf_camera_rays is its
    sdf_render, colours and step counts."""
    f = O.case_frame("C4-p1", name)
    want, wst = gpu_render(renderer, f, "C4-p1")
    o, d = renderer.camera_rays(f)
    out, st = renderer.render_rays(f, o.reshape(-1, 3), d.reshape(-1, 3), unit=True, steps=True)
    renderer.torch.cuda.synchronize()
    bad = (unequal(out.cpu().numpy().reshape(want.shape), want),
           unequal(st.cpu().numpy().reshape(wst.shape), wst))
    print(f"render_rays at {name}: words differing from the render (colour, steps) {bad}")
    assert bad == (0, 0)


# ---- meshes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mesh_equals_the_reference(renderer, name):
    """sdf_mesh_count and sdf_mesh_emit on a 24^3 grid around translated C4,
    with brick skipping and with SDF_MESH_DENSE: vertices, indices, normals and
    owners equal the NumPy reference over the oracle (tests/mesh_ref.py)."""
    f = O.case_frame("C4-p0", name)
    T = O.OFFSETS[name]
    origin = tuple(float(f32(v)) for v in np.array([-1.5, -0.25, -1.5]) + T)
    spec = (origin, 0.125, 24)
    ref = M.mesh(f, *spec)
    assert ref["counts"][0] > 300, ref["counts"]
    for dense in (False, True):
        got = raw_mesh(renderer, f, spec, dense=dense)
        bad = mismatches(got, ref) if got["counts"][:2] == ref["counts"] else None
        print(f"mesh at {name} dense={dense}: counts {got['counts']} reference {ref['counts']} "
              f"mismatches {bad}")
        assert got["counts"][:2] == ref["counts"]
        assert bad == {"verts": 0, "tris": 0, "normal": 0, "prim": 0}
        if dense:
            assert got["counts"][2] == got["counts"][3]


# ---- beyond the proven range ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["C4-p0", "C4-carved"])
def test_beyond_the_proven_range_the_frame_is_the_unculled_one(renderer, case):
    """Past 2^22 no plan culls (tests/test_offsets.py pins the boundary on the
    host): the default dispatch takes the generic kernel unculled, and the
    frame and its step counts are the oracle's and the unculled dispatch's."""
    f = O.translate(O.base_frame(case), np.array([0.0, 0.0, 2.0 ** 22 + 4.0]))
    assert O.bounds_of(f.scene)[3] == f.scene.count
    n0 = renderer.lib.sdf_jit_count()
    got, st = gpu_render(renderer, f, case)
    assert renderer.lib.sdf_jit_count() == n0          # no specialised kernel was asked for
    plain, pst = gpu_render(renderer, unculled(f), case)
    ref, rst = oracle.render(f)
    bad = (unequal(got, ref), unequal(st, rst), unequal(got, plain), unequal(st, pst))
    print(f"{case} beyond 2^22: words differing (oracle, its steps, unculled, its steps) {bad}")
    assert bad == (0, 0, 0, 0)
